"""Host references, yardsticks and the case lists of the attention edge tests (test_attention_ref_host.py on the CPU,
test_gpu_attention_edges.py on the GPU; tools/attention_edges.py writes the same cases' figures to profiles/attention_edges.txt).

Everything here is torch on the CPU.  The truth is `ref64` (float64 eager attention); a kernel's error on a case is `row_err` against it,
the worst (row, head) relative error, so one wrong row among hundreds is not diluted.  The bar of a case is a multiple of a yardstick
computed from the case's own inputs - `y32` (plain float32 eager attention) and, for the three-pass bf16 kernels, `y_split` (float64
attention on operands reduced to bf16 hi + lo, lo.lo dropped) - never from the kernel under test.

`make_case` builds inputs whose scores s_j = q.K_j / sqrt(128) follow a profile: q = randn + sqrt(128) u and K_j = randn + b_j u with a
unit vector u give s_j ~ b_j + N(0, 2 + b_j^2 / 128).  `online32` is the float32 tiled online softmax with a split combine that all six
kernels share, with switchable faults: the host test shows that each fault lands at least 10 x above the bar on some case of every
family's list, and that the fault-free form passes every case (the bar is neither blind nor too tight)."""
import functools
import math
from typing import NamedTuple

import torch

from oracle.qwen_decoder import rope_cos_sin

D = 128
EPS = 1e-6
PROFILES = ("flat", "shift+30", "shift-30", "shift+120", "shift-120", "ramp_up", "ramp_down", "sink", "saw", "newest")
FAULTS = ("newest_key_masked", "acc_not_rescaled", "l_not_rescaled", "combine_ignores_max", "gqa_modulo", "no_max_subtraction",
          "partial_tile_last_key_dropped")
MARGIN = 4.0                   # over a yardstick: one realisation of the rounding noise against another summation order, log2(e) folded
FLOOR_F32, FLOOR_SPLIT = 1e-5, 3e-5        # into the scale and v_exp_f32.  The floors are the suite's norm-wise bars, here per row
BAR_CAP = 5e-3                 # no case may need a looser bar than this: choose other inputs instead
THREE_PASS = ("bf16x3", "planes")
TILE = {"decode": 16, "verify": 16, "rows": 64, "mfma": 32, "bf16x3": 32, "planes": 32}     # keys per tile of the kernel family


# ---- the truth and the metric ------------------------------------------------------------------------------------------------------------
def _future(T, n_keys, pos0):
    return torch.arange(n_keys)[None, :] > (pos0 + torch.arange(T))[:, None]          # key j is visible to row t iff j <= pos0 + t


def _attn64(q, kc, vc, pos0):
    T, nq, _ = q.shape
    g = nq // kc.shape[0]
    n_keys = pos0 + T
    out = torch.zeros((T, nq, D), dtype=torch.float64)
    future = _future(T, n_keys, pos0)
    smax, smin = -math.inf, math.inf
    for h in range(nq):
        k, v = kc[h // g, :n_keys].double(), vc[h // g, :n_keys].double()
        s = (q[:, h].double() @ k.t()) / math.sqrt(D)
        vis = s[~future]
        smax, smin = max(smax, float(vis.max())), min(smin, float(vis.min()))
        out[:, h] = torch.softmax(s.masked_fill(future, -math.inf), dim=1) @ v
    return out, smax, smin


def ref64(q, kc, vc, pos0):
    """q [T, nq, 128] (rotated), caches [nkv, ctx, 128]: float64 eager causal GQA attention, one masked matrix product per head"""
    return _attn64(q, kc, vc, pos0)[0]


def row_err(got, want):
    """max over (t, h) of ||got - want||_2 / ||want||_2 over the 128 dims"""
    got, want = torch.as_tensor(got).double().reshape(want.shape), torch.as_tensor(want).double()
    return float(((got - want).norm(dim=-1) / want.norm(dim=-1).clamp_min(1e-300)).max())


# ---- yardsticks --------------------------------------------------------------------------------------------------------------------------
def eager32(q, kc, vc, pos0):
    """plain float32 eager attention: one float32 matmul per head, torch.softmax"""
    T, nq, _ = q.shape
    g = nq // kc.shape[0]
    n_keys = pos0 + T
    out = torch.zeros((T, nq, D), dtype=torch.float32)
    future = _future(T, n_keys, pos0)
    for h in range(nq):
        k, v = kc[h // g, :n_keys].float(), vc[h // g, :n_keys].float()
        s = (q[:, h].float() @ k.t()) / math.sqrt(D)
        out[:, h] = torch.softmax(s.masked_fill(future, -math.inf), dim=1) @ v
    return out


def _hi_lo(x):
    """x -> (bf16(x), bf16(x - bf16(x))) as float64: what a three-pass kernel keeps of an operand (about 17 mantissa bits)"""
    x = x.float()
    hi = x.to(torch.bfloat16).float()
    lo = (x - hi).to(torch.bfloat16).float()
    return hi.double(), lo.double()


def split64(q, kc, vc, pos0):
    """float64 attention on the operands of the declared three-pass arithmetic: q, K, V and the unnormalised P each as hi + lo, the
    products as hi.hi + hi.lo + lo.hi.  It models the arithmetic, not the kernels' code."""
    T, nq, _ = q.shape
    g = nq // kc.shape[0]
    n_keys = pos0 + T
    out = torch.zeros((T, nq, D), dtype=torch.float64)
    future = _future(T, n_keys, pos0)
    for h in range(nq):
        qh, ql = _hi_lo(q[:, h])
        kh, kl = _hi_lo(kc[h // g, :n_keys])
        vh, vl = _hi_lo(vc[h // g, :n_keys])
        s = (qh @ kh.t() + qh @ kl.t() + ql @ kh.t()) / math.sqrt(D)
        s = s.masked_fill(future, -math.inf)
        p = torch.exp(s - s.max(dim=1, keepdim=True).values)
        ph, pl = _hi_lo(p)
        out[:, h] = (ph @ vh + ph @ vl + pl @ vh) / p.sum(dim=1, keepdim=True)
    return out


# ---- the shared structure, with faults ---------------------------------------------------------------------------------------------------
def online32(q, kc, vc, pos0, tile, splits, fault=None):
    """float32 online softmax over tiles of `tile` keys; slot s walks tiles s, s + splits, ...; the slots' (m, l, acc) are merged by
    out = sum_s e^(m_s - M) acc_s / sum_s e^(m_s - M) l_s.  `fault` (one of FAULTS) breaks one step of it."""
    assert fault is None or fault in FAULTS
    q, kc, vc = q.float(), kc.float(), vc.float()
    T, nq, _ = q.shape
    nkv = kc.shape[0]
    g = nq // nkv
    head = torch.arange(nq) % nkv if fault == "gqa_modulo" else torch.arange(nq) // g
    n_keys = pos0 + T
    last = pos0 + torch.arange(T)                                    # newest visible key of each row
    keys = torch.arange(n_keys)
    hidden = keys[None, :] > last[:, None]
    if fault == "newest_key_masked":                                 # (a row whose only key is the newest keeps it: an empty row is
        hidden = hidden | ((keys[None, :] == last[:, None]) & (last[:, None] > 0))     # non-finite whatever else is right)
    if fault == "partial_tile_last_key_dropped":
        hidden = hidden | ((keys[None, :] == last[:, None]) & (last[:, None] > 0) & ((last[:, None] + 1) % tile != 0))
    scale = 1.0 / math.sqrt(D)
    n_tiles = (n_keys + tile - 1) // tile
    ms, ls, accs = [], [], []
    for slot in range(min(splits, n_tiles)):
        m = torch.full((T, nq), -math.inf)
        l = torch.zeros((T, nq))
        acc = torch.zeros((T, nq, D))
        for t0 in range(slot * tile, n_keys, splits * tile):
            t1 = min(t0 + tile, n_keys)
            s = torch.einsum("thd,hkd->thk", q, kc[head, t0:t1]) * scale
            s = s.masked_fill(hidden[:, None, t0:t1], -math.inf)
            if fault == "no_max_subtraction":
                m_new = torch.zeros_like(m)
                alpha = torch.ones_like(m)
            else:
                m_new = torch.maximum(m, s.max(dim=2).values)
                alpha = torch.where(m_new == -math.inf, torch.ones_like(m), torch.exp(m - m_new))   # no key seen yet: nothing to rescale
            p = torch.exp(s - torch.where(m_new == -math.inf, torch.zeros_like(m), m_new)[:, :, None])
            l = (l if fault == "l_not_rescaled" else l * alpha) + p.sum(dim=2)
            acc = (acc if fault == "acc_not_rescaled" else acc * alpha[:, :, None]) + torch.einsum("thk,hkd->thd", p, vc[head, t0:t1])
            m = m_new
        ms.append(m); ls.append(l); accs.append(acc)
    m, l, acc = torch.stack(ms), torch.stack(ls), torch.stack(accs)   # [slots, T, nq(, 128)]
    M = m.max(dim=0).values
    w = torch.where(m == -math.inf, torch.zeros_like(m), torch.exp(m - M[None]))         # a slot that saw no key of the row: weight 0
    if fault == "combine_ignores_max":
        w = (m > -math.inf).float()
    return (w[..., None] * acc).sum(dim=0) / (w * l).sum(dim=0)[..., None]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rope_tables(max_pos, theta=1e6):
    """the float32 tables the kernels read: (cos, sin) [max_pos, 64]"""
    cos, sin = rope_cos_sin(torch.arange(max_pos), D, theta)
    return cos[:, :64].contiguous(), sin[:, :64].contiguous()


def _rope64(x, pos, inverse=False):
    """x [T, heads, 128] float64 at positions pos [T]: NeoX rotate-half by the float32 tables, in float64"""
    cos, sin = rope_tables(int(pos.max()) + 1)
    c, s = cos[pos].double()[:, None, :], sin[pos].double()[:, None, :]
    if inverse:
        s = -s
    a, b = x[..., :64], x[..., 64:]
    return torch.cat([a * c - b * s, b * c + a * s], dim=-1)


def norm_rope64(raw, w, pos):
    """what the fused kernels do to a raw q / k head, in float64: optional RMSNorm (weights w [128]), then RoPE at pos"""
    x = raw.double()
    if w is not None:
        x = w.double() * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS))
    return _rope64(x, pos)


def offsets(profile, n_keys, pos0):
    """b_j of the profile for keys 0 .. n_keys - 1, and the |score| it aims at"""
    j = torch.arange(n_keys, dtype=torch.float64)
    if profile == "flat":
        return torch.zeros(n_keys, dtype=torch.float64), 0.0
    if profile.startswith("shift"):
        return torch.full((n_keys,), float(profile[5:]), dtype=torch.float64), abs(float(profile[5:]))
    if profile == "ramp_up":
        return 0.05 * j, 0.05 * (n_keys - 1)
    if profile == "ramp_down":
        return -0.05 * j, 0.05 * (n_keys - 1)
    if profile == "sink":
        return 8.0 * (j == 0), 8.0
    if profile == "saw":
        return 8.0 * ((j // 16) % 3 == 0), 8.0
    if profile == "newest":
        return 8.0 * (j >= pos0), 8.0
    raise ValueError(profile)


class Spec(NamedTuple):
    """one case: the kernel family, the score profile, u ("spread" or the one-hot dim), the shape and the options of the call"""
    family: str
    profile: str
    u: object
    nq: int
    nkv: int
    T: int
    pos0: int
    splits: int = 1
    max_ctx: int = 512
    f16: bool = False
    qk_norm: bool = False
    paged: int = 0            # block size of the paged form, 0: contiguous
    seed: int = 0
    norm_seed: object = None  # the q / k norm weights' seed when not the case's own (the sequences of a batched call share them)

    @property
    def fused(self):
        return self.family in ("decode", "verify")


def make_case(profile, u, nq, nkv, T, pos0, max_ctx, seed, f16=False, fused=False, qk_norm=False, norm_seed=None):
    """-> dict: q [T, nq, 128] float32 (rotated), k / v [nkv, max_ctx, 128] float32 holding the cache's values (fp16-representable
    when f16; NaN past the context), smax / smin / target (the realised extreme scores of ref64, and the profile's aim).
    fused: also raw [T, (nq + 2 nkv) * 128] (the un-rotated projections whose norm + RoPE are the targets: the inverse rotation in
    float64; with qk_norm the RMSNorm rescales them, which is accepted - its weights are drawn around the targets' rms), qn / kn,
    q64 and knew64 [T, nkv, 128] (the host's float64 norm + RoPE of raw); rows pos0 .. pos0 + T - 1 of k / v then hold what the
    kernel should write, and a test hands the kernel canaries there."""
    g = torch.Generator().manual_seed(seed)
    n_keys = pos0 + T
    if u == "spread":
        uv = torch.randn(D, generator=g, dtype=torch.float64)
        uv /= uv.norm()
    else:
        uv = torch.zeros(D, dtype=torch.float64)
        uv[int(u)] = 1.0
    b, target = offsets(profile, n_keys, pos0)
    q = torch.randn((T, nq, D), generator=g, dtype=torch.float64) + math.sqrt(D) * uv
    k = torch.randn((nkv, n_keys, D), generator=g, dtype=torch.float64)
    v = torch.randn((nkv, n_keys, D), generator=g, dtype=torch.float64)
    if profile == "flat" and n_keys > 17:
        k[:, 17] *= 4.0                                              # the suite's spiky key
    k = k + b[None, :, None] * uv
    case = dict(target=target, u=uv)
    if fused:
        pos = torch.arange(pos0, n_keys)
        qn = kn = None
        if qk_norm:                      # weights around the targets' own rms (q: sqrt(2); k: a shift's), so that the norm leaves their
            gw = torch.Generator().manual_seed(seed if norm_seed is None else norm_seed)       # scale alone; one pair for a whole batch
            # K_j = randn + b_j u has mean square 1 + b_j^2 / 128.  Only a shift moves every key by the same large b; ramp, sink,
            # saw and newest get 1.0 on purpose: their offsets differ per key (and are 0 or 8 for most), so no one weight scale
            # would undo the norm, and the norm flattening their larger keys is part of "the RMSNorm rescales the targets".
            shift = float(profile[5:]) if profile.startswith("shift") else 0.0
            qn = (math.sqrt(2.0) * (1 + 0.1 * torch.randn(D, generator=gw))).float()
            kn = (math.sqrt(1.0 + shift * shift / D) * (1 + 0.1 * torch.randn(D, generator=gw))).float()
        raw_q = _rope64(q, pos, inverse=True).float()
        raw_k = _rope64(k[:, pos0:].transpose(0, 1), pos, inverse=True).float()           # [T, nkv, 128]
        raw_v = v[:, pos0:].transpose(0, 1).float()
        case.update(raw=torch.cat([raw_q, raw_k, raw_v], dim=1).reshape(T, (nq + 2 * nkv) * D).contiguous(), qn=qn, kn=kn)
        q = norm_rope64(raw_q, qn, pos)
        knew = norm_rope64(raw_k, kn, pos)
        case.update(q64=q, knew64=knew)
        k[:, pos0:] = knew.transpose(0, 1)
        v[:, pos0:] = raw_v.double().transpose(0, 1)
    store = (lambda x: x.half().float()) if f16 else (lambda x: x.float())
    kc = torch.full((nkv, max_ctx, D), float("nan"))
    vc = torch.full((nkv, max_ctx, D), float("nan"))
    kc[:, :n_keys] = store(k)
    vc[:, :n_keys] = store(v)
    case.update(q=q.float(), k=kc, v=vc)
    _, case["smax"], case["smin"] = _attn64(case["q"], kc, vc, pos0)
    return case


def bar_of(family, y32, y_split):
    if family in THREE_PASS:
        return max(MARGIN * max(y32, y_split), FLOOR_SPLIT)
    return max(MARGIN * y32, FLOOR_F32)


@functools.lru_cache(maxsize=64)
def build(spec):
    """the case of a Spec with its truth and yardsticks: want (ref64 on the host's inputs), y32, y_split, bar"""
    c = make_case(spec.profile, spec.u, spec.nq, spec.nkv, spec.T, spec.pos0, spec.max_ctx, spec.seed, spec.f16, spec.fused, spec.qk_norm,
                  spec.norm_seed)
    c["want"] = ref64(c["q"], c["k"], c["v"], spec.pos0)
    c["y32"] = row_err(eager32(c["q"], c["k"], c["v"], spec.pos0), c["want"])
    c["y_split"] = row_err(split64(c["q"], c["k"], c["v"], spec.pos0), c["want"]) if spec.family in THREE_PASS else 0.0
    c["bar"] = bar_of(spec.family, c["y32"], c["y_split"])
    return c


# ---- the case lists (shared by the host test, the GPU test and tools/attention_edges.py) -------------------------------------------------
US = ("spread", 5, 69)        # one-hot at dim 5 and at dim 69: the fp16 K layout splits the dims at 64
DECODE_POS = (0, 15, 16, 17, 333, -1)        # tile edges of the 16-key tiles, several tiles, a parked sequence


class DecodeBatch(NamedTuple):
    """one batched decode call: a sequence per position (each with a cache of its own), -1 = parked"""
    profile: str
    u: object
    group: int
    splits: int
    f16: bool
    qk_norm: bool
    paged: int = 0
    positions: tuple = DECODE_POS
    max_ctx: int = 512
    nkv: int = 2
    seed: int = 0

    def specs(self):
        return [Spec("decode", self.profile, self.u, self.nkv * self.group, self.nkv, 1, p, self.splits, self.max_ctx, self.f16,
                     self.qk_norm, self.paged, self.seed * 16 + i, self.seed) for i, p in enumerate(self.positions) if p >= 0]


def _decode_batches():
    out, i = [], 0
    # groups 1 .. 8 on flat and shift+120, both caches (launch_decode: <4,false> for 1 - 3, <4,true>, <5,true>, <6,false>, <8,false> for 7, 8).
    # Group 1 runs on 8 kv heads: a sequence is one case with its own yardstick, and with two heads that yardstick is the larger of two
    # draws of the rounding noise - the fault-free float32 form itself came out 4.5 x above it (pos 17, shift+120, fp16).  Eight rows
    # make the worst row of one float32 realisation stand for another's.
    for group in range(1, 9):
        for profile in ("flat", "shift+120"):
            for f16 in (False, True):
                out.append(DecodeBatch(profile, US[i % 3], group, (1, 3, 64)[(i // 2) % 3], f16, bool((i // 6) % 2), nkv=8 if group == 1 else 2,
                                       seed=1000 + i))
                i += 1
    # the shipped groups and the widest one on every profile, every (splits, qk_norm) pair
    for group in (4, 5, 8):
        for profile in PROFILES:
            for f16 in (False, True):
                out.append(DecodeBatch(profile, US[i % 3], group, (1, 3, 64)[i % 3], f16, bool((i // 3) % 2), seed=1000 + i))
                i += 1
    for f16 in (False, True):                                        # block-paged, 64-row blocks
        out.append(DecodeBatch("shift+120", 69, 5, 3, f16, True, paged=64, seed=1000 + i))
        i += 1
    return out


def _decode_long():
    """pos 4095 of 4096: 256 tiles through one slot's ping-pong (splits 1), 4 tiles in each of 64 slots"""
    out, i = [], 0
    for profile in ("ramp_up", "shift+120"):
        for splits in (1, 64):
            for f16 in (False, True):
                out.append(DecodeBatch(profile, US[i % 3], 5, splits, f16, False, positions=(4095,), max_ctx=4096, seed=2000 + i))
                i += 1
    return out


def _verify_specs():
    out, i = [], 0
    todo = [(g, p) for g in (1, 3, 6, 7, 8) for p in ("flat", "shift+120")] + [(5, p) for p in PROFILES]
    for group, profile in todo:
        for R in (2, 9):
            for pos in (0, 15, 200):
                for f16 in (False, True):
                    out.append(Spec("verify", profile, US[i % 3], 2 * group, 2, R, pos, (1, 2, 4, 16)[i % 4], 512, f16, bool((i // 4) % 2),
                                    seed=3000 + i))
                    i += 1
    return out


def _rows_specs():
    out, i = [], 0
    for nq, nkv in ((6, 2), (12, 2), (7, 1)):                        # groups 3, 6, 7
        for T in (1, 7):
            for pos0 in (0, 63, 333):
                for splits in (1, 4, 16):
                    out.append(Spec("rows", ("flat", "shift+120")[i % 2], US[(i // 2) % 3], nq, nkv, T, pos0, splits, seed=4000 + i))
                    i += 1
    for profile in PROFILES:
        for T in (1, 7):
            for pos0 in (0, 63, 333):
                out.append(Spec("rows", profile, US[i % 3], 10, 2, T, pos0, (1, 4, 16)[i % 3], f16=bool(i % 2), seed=4000 + i))
                i += 1
    return out


def _prefill_specs(family):
    """bf16x3 / float32-MFMA: every (T, pos0, splits) on flat or shift+120 and on one more profile, all profiles in turn, at (10, 2).
    splits 2 and 4 at T = 16, pos0 = 0 leave slots with no key for any row, at T = 130 slots that only the later rows see."""
    out, i = [], 0
    for T in (16, 65, 130):
        for pos0 in (0, 31, 300):
            for splits in (1, 2, 4):
                for profile in dict.fromkeys((("flat", "shift+120")[i % 2], PROFILES[i % 10])):
                    out.append(Spec(family, profile, US[len(out) % 3], 10, 2, T, pos0, splits, seed=5000 + len(out)))
                i += 1
    return out


def _planes_specs():
    out, i = [], 0
    # n_kv 3 and 6 do not divide 8: the plain workgroup order; 1, 2, 4, 8: one kv head over 8, 4, 2, 1 XCDs (4 = the TP = 2 shard)
    for nkv, group in ((1, 5), (2, 3), (3, 2), (4, 2), (6, 1), (8, 1)):
        for T in (64, 130):
            for profile in ("flat", "shift+120"):
                out.append(Spec("planes", profile, US[i % 3], nkv * group, nkv, T, (0, 31, 300)[i % 3], seed=6000 + i))
                i += 1
    for profile in PROFILES:
        for T in (64, 130):
            out.append(Spec("planes", profile, US[i % 3], 10, 2, T, (0, 31, 300)[i % 3], seed=6000 + i))
            i += 1
    return out


def _long_prefill_specs():
    """T = 64 at pos0 = 4032 of 4096 (no ramp here: 0.05 x 4095 is past the |s| = 120 the three-pass bar can follow)"""
    return [Spec(family, profile, u, 10, 2, 64, 4032, 1, 4096, paged=paged, seed=7000 + i)
            for i, (family, profile, u, paged) in enumerate([("planes", "saw", "spread", 0), ("planes", "shift+120", 69, 64),
                                                             ("bf16x3", "saw", "spread", 0), ("bf16x3", "shift+120", 69, 64)])]


DECODE_BATCHES = _decode_batches()
DECODE_LONG = _decode_long()
VERIFY = _verify_specs()
ROWS = _rows_specs()
PREFILL = {f: _prefill_specs(f) for f in ("bf16x3", "mfma")}
PLANES = _planes_specs()
LONG_PREFILL = _long_prefill_specs()
PLANES_XCD_AB = [Spec("planes", "shift+120", 5, nkv * 2, nkv, 130, 31, seed=6500 + nkv) for nkv in (2, 4)]



# the common score offset S = 0 / 30 / 120 along a spread and a one-hot direction, one shape per kernel, all at (10, 2) - decode: group 5,
# the batch's positions, 3 slots; verify: 9 rows at pos 200, 4 slots; rows: T = 7 at pos0 = 333, 4 slots; prefill kernels: T = 64 at
# pos0 = 100 (two slots for the kernels that have a combine).  DESIGN.md's table of error against score magnitude is read off these.
SWEEP_S = (("flat", 0), ("shift+30", 30), ("shift+120", 120))
SWEEP_U = ("spread", 5)
SWEEP_DECODE, SWEEP = [], []
for _profile, _S in SWEEP_S:
    for _u in SWEEP_U:
        _seed = 9000 + _S + (0 if _u == "spread" else 1)
        SWEEP_DECODE.append(DecodeBatch(_profile, _u, 5, 3, False, False, seed=_seed))
        SWEEP += [Spec("verify", _profile, _u, 10, 2, 9, 200, 4, seed=_seed), Spec("rows", _profile, _u, 10, 2, 7, 333, 4, seed=_seed),
                  Spec("mfma", _profile, _u, 10, 2, 64, 100, 2, seed=_seed), Spec("bf16x3", _profile, _u, 10, 2, 64, 100, 2, seed=_seed),
                  Spec("planes", _profile, _u, 10, 2, 64, 100, 1, seed=_seed)]
ALL_DECODE = DECODE_BATCHES + SWEEP_DECODE + DECODE_LONG             # (the long cases last)


def family_specs():
    """family -> every Spec the GPU test and the tool run on it"""
    long = {f: [s for s in LONG_PREFILL if s.family == f] for f in ("planes", "bf16x3")}
    sweep = {f: [s for s in SWEEP if s.family == f] for f in TILE}
    return {"decode": [s for b in ALL_DECODE for s in b.specs()], "verify": VERIFY + sweep["verify"], "rows": ROWS + sweep["rows"],
            "bf16x3": PREFILL["bf16x3"] + sweep["bf16x3"] + long["bf16x3"], "mfma": PREFILL["mfma"] + sweep["mfma"],
            "planes": PLANES + PLANES_XCD_AB + sweep["planes"] + long["planes"]}


def build_batch(batch):
    """the cases of one batched decode call, one per live sequence, each with its own yardstick and bar"""
    return [build(s) for s in batch.specs()]


def iter_cases(family):
    """(spec, case, bar) of every case the GPU test and the tool run on the family"""
    for spec in family_specs()[family]:
        c = build(spec)
        yield spec, c, c["bar"]
