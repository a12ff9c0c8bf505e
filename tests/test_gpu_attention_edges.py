"""Every attention kernel against float64 PER ROW on model-like score ranges and on the head layouts no other test executes.

The cases, the float64 truth (`ref64`), the metric (`row_err`: the worst (row, head) relative error over the 128 dims) and the bars come
from tests/attention_ref.py; test_attention_ref_host.py shows on the CPU that every case reaches its score range, that a fault-free
float32 online softmax passes every bar and that each of seven planted faults lands 10 x above it.  A case's bar is a multiple of a
yardstick computed on the host from the case's own inputs, never from the kernel: max(4 y32, 1e-5) for the float32-arithmetic kernels
(rows, decode, verify, float32-MFMA), max(4 max(y32, y_split), 3e-5) for the three-pass bf16 kernels (bf16x3, planes).  A sequence of a
batched decode call is a case of its own.  tools/attention_edges.py runs the same cases through the functions of this file and writes
each one's error, yardsticks and ratio to profiles/attention_edges.txt.

Asserted in every case, besides err <= bar: the output is finite (the partials' workspace starts as NaN: nothing may be read that the
call did not write), cache rows outside the written range keep their bits (NaN canaries past the context), the new K rows of the fused
kernels equal the host's float64 norm + RoPE from the float32 tables to 1e-6 norm-wise (test_rope_kv_write's bar; on the fp16 cache
plus fp16's unit roundoff 2^-11: the row IS the rounding), the V rows are the input's bits.  The reference of the fused kernels is the
host's float64 rotated q on K / V read back from the cache after the call.

Paths that no other test executes, and the cases that do here:
  launch_decode <4,false> with 1 - 3 heads, <6,false>, <kMaxGroup,false> at 7, group 8 on the float32 cache
                                                   test_decode_groups_1_to_8 (ar.DECODE_BATCHES[:32]: every group on both caches)
  attn_verify_kernel with groups 1, 3, 6, 7, 8     test_verify_groups_1_3_6_7_8 (the first 120 of ar.VERIFY)
  attn_prefill_planes_kernel, plain workgroup order  test_planes_kv_head_counts at n_kv 3 and 6 (ar.PLANES), test_planes_xcd_order_is_bitwise
                                                   under option ATTN_XCD=0 (ar.PLANES_XCD_AB)
  attn_prefill_planes_kernel at n_kv = 4           test_planes_kv_head_counts, test_planes_xcd_order_is_bitwise
  attn_rows_kernel with groups 3, 6, 7             test_rows_groups_3_6_7 (the first 54 of ar.ROWS: (6, 2), (12, 2), (7, 1))
  contexts above 1024 keys                         test_decode_long (pos 4095 of 4096), test_prefill_long (pos0 4032 of 4096)"""
import ctypes as C
from typing import NamedTuple

import pytest
import torch

from chatts_amd import _lib
from tests import attention_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return _lib.load()

K_ROW_TOL = 1e-6
F16_ROUNDOFF = 2.0 ** -11


def st():
    return _lib.stream_ptr()


class Rec(NamedTuple):
    kernel: str
    what: str
    err: float
    y32: float
    y_split: float
    bar: float
    smax: float
    smin: float

    @property
    def ratio(self):
        return self.err / max(self.y32, self.y_split, 1e-30)

    @property
    def ok(self):
        return self.err <= self.bar

    def line(self):
        return (f"{self.kernel:7s} {self.err:9.3g} {self.y32:9.3g} {self.y_split:9.3g} {self.ratio:6.2f} {self.bar:9.3g} {self.smin:7.1f} "
                f"{self.smax:7.1f}  {self.what}" + ("" if self.ok else "   ABOVE THE BAR"))


def _what(s, T=None, pos=None):
    return (f"{s.profile} u={s.u} nq={s.nq} nkv={s.nkv} T={s.T if T is None else T} pos={s.pos0 if pos is None else pos} splits={s.splits} "
            f"ctx={s.max_ctx}{' f16' if s.f16 else ''}{' qk_norm' if s.qk_norm else ''}{' paged' if s.paged else ''}")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _nan_bytes(n):
    return torch.full((max(n, 16),), 0xFF, dtype=torch.uint8, device=DEV)


def _tables(max_ctx):
    cos, sin = ar.rope_tables(max_ctx)
    return cos.to(DEV), sin.to(DEV)


def _pool(caches, block, seed):
    """caches [B, nkv, max_ctx, 128] (K or V of B sequences) -> one pool [B * nb + 3, nkv, block, 128] with the logical blocks of all
    sequences shuffled through it (spares: NaN), table [B, nb] int32"""
    B, nkv, max_ctx, _ = caches.shape
    nb = max_ctx // block
    table = torch.randperm(B * nb + 3, generator=torch.Generator().manual_seed(seed))[:B * nb].view(B, nb)
    pool = torch.full((B * nb + 3, nkv, block, ar.D), float("nan"), dtype=caches.dtype, device=caches.device)
    pool[table.reshape(-1)] = caches.view(B, nkv, nb, block, ar.D).transpose(1, 2).reshape(B * nb, nkv, block, ar.D)
    return pool, table.to(torch.int32).to(caches.device)


def _unpool(pool, table):
    B, nb = table.shape
    x = pool[table.reshape(-1).long()]                                                 # [B * nb, nkv, block, 128]
    return x.view(B, nb, *x.shape[1:]).transpose(1, 2).reshape(B, x.shape[1], -1, ar.D)


class _Cache:
    """K / V of B sequences on the device as the call sees them (contiguous or one shared pool), and back as [B, nkv, max_ctx, 128]"""

    def __init__(self, k, v, f16, block, seed):
        dt = torch.float16 if f16 else torch.float32
        self.k0, self.v0 = k.to(DEV).to(dt), v.to(DEV).to(dt)
        self.block = block
        max_ctx = k.shape[2]
        if block:
            self.pk, self.table = _pool(self.k0, block, seed)
            self.pv, _ = _pool(self.v0, block, seed)
            self.arg = _lib.KvCache(k=self.pk.data_ptr(), v=self.pv.data_ptr(), max_ctx=max_ctx, dtype=int(f16), block_table=self.table.data_ptr(),
                                    block_size=block, table_stride=self.table.shape[1])
            self.seq_stride = 0
        else:
            self.pk, self.pv = self.k0.clone(), self.v0.clone()
            self.arg = _lib.KvCache(k=self.pk.data_ptr(), v=self.pv.data_ptr(), max_ctx=max_ctx, dtype=int(f16))
            self.seq_stride = k.shape[1] * max_ctx * ar.D

    def read(self):
        if not self.block:
            return self.pk, self.pv
        spare = torch.ones(self.pk.shape[0], dtype=torch.bool)
        spare[self.table.reshape(-1).long().cpu()] = False
        spare = spare.to(DEV)
        assert torch.isnan(self.pk[spare]).all() and torch.isnan(self.pv[spare]).all()       # blocks outside the table: not written
        return _unpool(self.pk, self.table), _unpool(self.pv, self.table)


def _check_new_rows(spec, c, k_after, v_after, pos):
    """rows pos .. pos + T - 1 of one sequence's cache [nkv, max_ctx, 128] against the host: K norm + RoPE in float64, V the input's bits"""
    T = spec.T
    got_k = k_after[:, pos:pos + T].float().cpu().double().transpose(0, 1)              # [T, nkv, 128]
    want_k = c["knew64"]
    err = float((got_k - want_k).norm() / want_k.norm())
    assert err <= K_ROW_TOL + (F16_ROUNDOFF if spec.f16 else 0.0), (spec, err)
    want_v = c["raw"].view(T, spec.nq + 2 * spec.nkv, ar.D)[:, spec.nq + spec.nkv:].transpose(0, 1)
    assert _same_bits(v_after[:, pos:pos + T].cpu(), want_v.half() if spec.f16 else want_v), spec


# ---- decode --------------------------------------------------------------------------------------------------------------------------
def measure_decode(lib, batch):
    """one chatts_attention_decode_batched call (chatts_attention_decode_fused when the batch is a single sequence) -> a Rec per live
    sequence: each sequence is a case with its own yardstick and bar"""
    specs, cases = batch.specs(), ar.build_batch(batch)
    live = [b for b, p in enumerate(batch.positions) if p >= 0]
    B, nkv, nq, max_ctx = len(batch.positions), batch.nkv, batch.nkv * batch.group, batch.max_ctx
    raw = torch.full((B, (nq + 2 * nkv) * ar.D), float("nan"))
    k = torch.full((B, nkv, max_ctx, ar.D), float("nan"))
    v = torch.full((B, nkv, max_ctx, ar.D), float("nan"))
    for b, s, c in zip(live, specs, cases):
        raw[b] = c["raw"][0]
        k[b, :, :s.pos0] = c["k"][:, :s.pos0]                       # the context; the new row and everything after it: canaries
        v[b, :, :s.pos0] = c["v"][:, :s.pos0]
    cache = _Cache(k, v, batch.f16, batch.paged, batch.seed)
    raw_d = raw.to(DEV)
    qn, kn = (cases[0]["qn"].to(DEV), cases[0]["kn"].to(DEV)) if batch.qk_norm else (None, None)
    assert not batch.qk_norm or all(torch.equal(c["kn"], cases[0]["kn"]) and torch.equal(c["qn"], cases[0]["qn"]) for c in cases)
    cos, sin = _tables(max_ctx)
    wsb = int(lib.chatts_attn_workspace(B, nq, batch.splits))
    ws = _nan_bytes(wsb)
    out = torch.full((B, nq * ar.D), float("nan"), device=DEV)
    if B == 1:
        _lib.check(lib.chatts_attention_decode_fused(raw_d.data_ptr(), nq, nkv, _lib.ptr(qn), _lib.ptr(kn), ar.EPS, cos.data_ptr(), sin.data_ptr(),
                                                     batch.positions[0], None, C.byref(cache.arg), out.data_ptr(), batch.splits, ws.data_ptr(),
                                                     wsb, st()))
    else:
        pos_dev = torch.tensor(batch.positions, dtype=torch.int32, device=DEV)
        _lib.check(lib.chatts_attention_decode_batched(raw_d.data_ptr(), B, nq, nkv, _lib.ptr(qn), _lib.ptr(kn), ar.EPS, cos.data_ptr(),
                                                       sin.data_ptr(), 0, pos_dev.data_ptr(), C.byref(cache.arg), cache.seq_stride,
                                                       out.data_ptr(), batch.splits, ws.data_ptr(), wsb, st()))
    torch.cuda.synchronize()
    ka, va = cache.read()
    out = out.cpu().view(B, nq, ar.D)
    recs = []
    for b, p in enumerate(batch.positions):
        if p < 0:                                                    # parked: nothing written, the output row is zeros
            assert _same_bits(ka[b], cache.k0[b]) and _same_bits(va[b], cache.v0[b]) and bool((out[b] == 0).all()), batch
            continue
        s, c = specs[live.index(b)], cases[live.index(b)]
        assert torch.isfinite(out[b]).all(), s
        assert _same_bits(ka[b, :, :p], cache.k0[b, :, :p]) and _same_bits(va[b, :, :p], cache.v0[b, :, :p]), s
        assert torch.isnan(ka[b, :, p + 1:]).all() and torch.isnan(va[b, :, p + 1:]).all(), s
        _check_new_rows(s, c, ka[b], va[b], p)
        want = ar.ref64(c["q64"], ka[b].float().cpu(), va[b].float().cpu(), p)
        recs.append(Rec("decode", _what(s) + f" seq {b}/{B}", ar.row_err(out[b:b + 1], want), c["y32"], 0.0, c["bar"], c["smax"], c["smin"]))
    return recs


# ---- verify --------------------------------------------------------------------------------------------------------------------------
def measure_verify(lib, spec):
    c = ar.build(spec)
    R, nq, nkv, pos = spec.T, spec.nq, spec.nkv, spec.pos0
    k, v = c["k"].clone(), c["v"].clone()
    k[:, pos:] = float("nan")                                        # the in-flight rows come from qkv, never from the cache
    v[:, pos:] = float("nan")
    cache = _Cache(k[None], v[None], spec.f16, spec.paged, spec.seed)
    raw = c["raw"].to(DEV)
    qn, kn = (c["qn"].to(DEV), c["kn"].to(DEV)) if spec.qk_norm else (None, None)
    cos, sin = _tables(spec.max_ctx)
    wsb = int(lib.chatts_attn_workspace(R, nq, spec.splits))
    ws = _nan_bytes(wsb)
    out = torch.full((R, nq * ar.D), float("nan"), device=DEV)
    pos_dev = torch.tensor([pos], dtype=torch.int32, device=DEV)
    _lib.check(lib.chatts_attention_verify(raw.data_ptr(), R, nq, nkv, _lib.ptr(qn), _lib.ptr(kn), ar.EPS, cos.data_ptr(), sin.data_ptr(),
                                           pos_dev.data_ptr(), C.byref(cache.arg), out.data_ptr(), spec.splits, ws.data_ptr(), wsb, st()))
    torch.cuda.synchronize()
    ka, va = (x[0] for x in cache.read())
    out = out.cpu().view(R, nq, ar.D)
    assert torch.isfinite(out).all(), spec
    assert _same_bits(ka[:, :pos], cache.k0[0, :, :pos]) and _same_bits(va[:, :pos], cache.v0[0, :, :pos]), spec
    assert torch.isnan(ka[:, pos + R:]).all() and torch.isnan(va[:, pos + R:]).all(), spec
    _check_new_rows(spec, c, ka, va, pos)
    want = ar.ref64(c["q64"], ka.float().cpu(), va.float().cpu(), pos)
    return Rec("verify", _what(spec), ar.row_err(out, want), c["y32"], 0.0, c["bar"], c["smax"], c["smin"])


# ---- rows / prefill / planes ---------------------------------------------------------------------------------------------------------
def plane_bytes(spec):
    return ((spec.pos0 + spec.T + 31) // 32) * spec.nkv * 4 * 32 * ar.D * 2


def run_attention(lib, spec, c):
    """chatts_attention on the case's cache -> out [T, nq, 128] on the host.  The family picks the kernel: `planes` hands over a
    workspace of exactly plane_bytes, the others none beyond the partials of splits > 1 (so bf16x3 splits while it stages)."""
    T, nq, nkv, pos0 = spec.T, spec.nq, spec.nkv, spec.pos0
    cache = _Cache(c["k"][None], c["v"][None], spec.f16, spec.paged, spec.seed)
    qkv = torch.cat([c["q"].reshape(T, nq * ar.D), torch.full((T, 2 * nkv * ar.D), float("nan"))], dim=1).to(DEV)    # only q is read
    if spec.family == "planes":
        wsb = plane_bytes(spec)
    else:
        wsb = int(lib.chatts_attn_workspace(T, nq, spec.splits)) if spec.splits > 1 else 0
    ws = _nan_bytes(wsb)
    out = torch.full((T, nq * ar.D), float("nan"), device=DEV)
    _lib.check(lib.chatts_attention(qkv.data_ptr(), T, nq, nkv, pos0, None, C.byref(cache.arg), out.data_ptr(), spec.splits,
                                    ws.data_ptr() if wsb else None, wsb, st()))
    torch.cuda.synchronize()
    if spec.family == "planes":
        assert not bool((ws == 0xFF).all()), spec                    # the planes really were written: that kernel ran
    ka, va = cache.read()
    assert _same_bits(ka, cache.k0) and _same_bits(va, cache.v0), spec                  # the cache is only read; canaries intact
    out = out.cpu().view(T, nq, ar.D)
    assert torch.isfinite(out).all(), spec
    return out


KERNEL_OPTIONS = {"rows": {}, "mfma": {"ATTN_BF16X3": 0}, "bf16x3": {"ATTN_BF16X3": 1}, "planes": {"ATTN_BF16X3": 1}}


def measure_attention(lib, spec):
    c = ar.build(spec)
    with _lib.options(**KERNEL_OPTIONS[spec.family]):
        out = run_attention(lib, spec, c)
    return Rec(spec.family, _what(spec), ar.row_err(out, c["want"]), c["y32"], c["y_split"], c["bar"], c["smax"], c["smin"])


def measure_xcd_ab(lib, spec):
    """-> Rec of the plain order, after asserting: each (query tile, head) work item performs the same arithmetic whichever workgroup
    runs it, ATTN_XCD=0 == the XCD-aware order bit for bit"""
    c = ar.build(spec)
    outs = []
    for xcd in (1, 0):
        with _lib.options(ATTN_BF16X3=1, ATTN_XCD=xcd):
            outs.append(run_attention(lib, spec, c))
    assert _same_bits(outs[0], outs[1]), spec
    return Rec("planes", _what(spec) + " XCD=1 == XCD=0", ar.row_err(outs[1], c["want"]), c["y32"], c["y_split"], c["bar"], c["smax"],
               c["smin"])


# ---- the tests ------------------------------------------------------------------------------------------------------------------------
def assert_within_bars(recs):
    """print every figure, then: no case above its bar"""
    recs = list(recs)
    for r in recs:
        print(r.line())
    over = [r.line() for r in recs if not r.ok]
    assert recs and not over, "\n" + "\n".join(over)


N_GROUP_BATCHES = 8 * 2 * 2          # ar.DECODE_BATCHES opens with groups 1 .. 8 x (flat, shift+120) x (float32, fp16)
N_VERIFY_GROUPS = 5 * 2 * 2 * 3 * 2  # ar.VERIFY opens with groups (1, 3, 6, 7, 8) x (flat, shift+120) x R x pos x cache
N_ROWS_GROUPS = 3 * 2 * 3 * 3        # ar.ROWS opens with (6, 2), (12, 2), (7, 1) x T x pos0 x splits


def test_decode_groups_1_to_8(lib):
    """chatts_attention_decode_batched, groups 1 .. 8 on flat and shift+120, both caches, positions 0 / 15 / 16 / 17 / 333 and a parked
    sequence in one batch, splits 1 / 3 / 64, qk_norm on and off: every instantiation launch_decode picks, <4,false> with 1 - 3 heads
    (group 1 on 8 kv heads), <6,false>, <kMaxGroup,false> at 7 and 8 on both caches among them"""
    batches = ar.DECODE_BATCHES[:N_GROUP_BATCHES]
    assert {(b.group, b.f16) for b in batches} == {(g, f) for g in range(1, 9) for f in (False, True)}
    assert_within_bars(r for b in batches for r in measure_decode(lib, b))


def test_decode_every_profile(lib):
    """groups 4, 5 and 8 on every profile and both caches, and the block-paged form (64-row blocks)"""
    batches = ar.DECODE_BATCHES[N_GROUP_BATCHES:]
    assert {b.profile for b in batches} == set(ar.PROFILES) and any(b.paged for b in batches)
    assert_within_bars(r for b in batches for r in measure_decode(lib, b))


def test_decode_long(lib):
    """chatts_attention_decode_fused at pos 4095 of 4096: 256 tiles through one slot's ping-pong (splits 1), 4 tiles in each of 64 slots"""
    assert all(b.positions == (4095,) for b in ar.DECODE_LONG)
    assert_within_bars(r for b in ar.DECODE_LONG for r in measure_decode(lib, b))


def test_verify_groups_1_3_6_7_8(lib):
    """attn_verify_kernel with the groups no other test runs, on flat and shift+120, R 2 / 9, pos 0 / 15 / 200, both caches"""
    specs = ar.VERIFY[:N_VERIFY_GROUPS]
    assert {s.nq // s.nkv for s in specs} == {1, 3, 6, 7, 8}
    assert_within_bars(measure_verify(lib, s) for s in specs)


def test_verify_every_profile(lib):
    specs = ar.VERIFY[N_VERIFY_GROUPS:]
    assert {s.nq // s.nkv for s in specs} == {5} and {s.profile for s in specs} == set(ar.PROFILES)
    assert_within_bars(measure_verify(lib, s) for s in specs)


def test_rows_groups_3_6_7(lib):
    """attn_rows_kernel (chatts_attention, T < 16) at (6, 2), (12, 2), (7, 1): T 1 / 7, pos0 0 / 63 / 333, splits 1 / 4 / 16"""
    specs = ar.ROWS[:N_ROWS_GROUPS]
    assert {s.nq // s.nkv for s in specs} == {3, 6, 7}
    assert_within_bars(measure_attention(lib, s) for s in specs)


def test_rows_every_profile(lib):
    specs = ar.ROWS[N_ROWS_GROUPS:]
    assert {(s.nq, s.nkv) for s in specs} == {(10, 2)} and {s.profile for s in specs} == set(ar.PROFILES)
    assert_within_bars(measure_attention(lib, s) for s in specs)


@pytest.mark.parametrize("family", ["mfma", "bf16x3"])
def test_prefill_every_profile(lib, family):
    """float32-MFMA (option ATTN_BF16X3=0) and bf16x3 (=1, no workspace for planes) prefill at (10, 2): T 16 / 65 / 130, pos0 0 / 31 / 300,
    splits 1 / 2 / 4 (slots that no row, or only the later rows, see a key of), every profile"""
    specs = ar.PREFILL[family]
    assert {s.profile for s in specs} == set(ar.PROFILES)
    assert_within_bars(measure_attention(lib, s) for s in specs)


def test_planes_kv_head_counts(lib):
    """attn_prefill_planes_kernel (workspace exactly plane_bytes) at n_kv 1, 2, 3, 4, 6, 8 - 3 and 6 do not divide 8: the plain workgroup
    order; 4: two XCDs per kv head - and every profile at (10, 2)"""
    assert {s.nkv for s in ar.PLANES} == {1, 2, 3, 4, 6, 8} and {s.profile for s in ar.PLANES} == set(ar.PROFILES)
    assert_within_bars(measure_attention(lib, s) for s in ar.PLANES)


def test_planes_xcd_order_is_bitwise(lib):
    """option ATTN_XCD=0 (the plain order) at n_kv 2 and 4 equals the XCD-aware order bit for bit, and both hold the bar"""
    assert [s.nkv for s in ar.PLANES_XCD_AB] == [2, 4]
    assert_within_bars(measure_xcd_ab(lib, s) for s in ar.PLANES_XCD_AB)


def test_prefill_long(lib):
    """T = 64 at pos0 = 4032 of 4096 on the planes and the bf16x3 kernel, contiguous and block-paged"""
    assert {(s.family, bool(s.paged)) for s in ar.LONG_PREFILL} == {(f, p) for f in ("planes", "bf16x3") for p in (False, True)}
    assert_within_bars(measure_attention(lib, s) for s in ar.LONG_PREFILL)


def test_score_offset_sweep(lib):
    """the common score offset S = 0 / 30 / 120 along a spread and a one-hot direction at one shape per kernel: the cases behind
    DESIGN.md's table of error against score magnitude"""
    assert_within_bars([r for b in ar.SWEEP_DECODE for r in measure_decode(lib, b)]
                       + [(measure_verify if s.family == "verify" else measure_attention)(lib, s) for s in ar.SWEEP])
