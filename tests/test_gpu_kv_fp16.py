"""GPU: the fp16 KV cache (ChattsKvCache.dtype = CHATTS_KV_F16, ChatTSForCausalLM(kv_cache_dtype="fp16")).

The float32 reference of every check is the same call on a float32 cache holding the widened fp16 values, or the float32 path under
option KV_ROUND=3 (which rounds K / V to fp16 values as they enter the float32 cache): the writes and the K / V planes must match it
bit for bit, the attention kernels (which may sum a score's dims in another order) to 1e-6, and a float64 restatement on the fp16
values to the suite's 1e-5.  Rows past the context hold fp16 NaN canaries: nothing may read them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from chatts_amd import _lib
from tests.util import chat_prompt, random_walk_series, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _lib.load()


def st():
    return _lib.stream_ptr()


def _rope_tables(max_pos, theta=1e6):
    from oracle.qwen_decoder import rope_cos_sin
    cos, sin = rope_cos_sin(torch.arange(max_pos), 128, theta)
    return cos[:, :64].contiguous().to(DEV), sin[:, :64].contiguous().to(DEV)


def _ref_attention(q, kc, vc, pos0):
    """q [T, nq, 128] (rotated), caches [nkv, ctx, 128]: float64 causal GQA attention"""
    T, nq, _ = q.shape
    g = nq // kc.shape[0]
    n_keys = pos0 + T
    out = torch.zeros((T, nq, 128), dtype=torch.float64)
    future = torch.arange(n_keys)[None, :] > (pos0 + torch.arange(T))[:, None]
    for h in range(nq):
        k, v = kc[h // g, :n_keys].double(), vc[h // g, :n_keys].double()
        s = ((q[:, h].double() @ k.t()) / np.sqrt(128.0)).masked_fill(future, float("-inf"))
        out[:, h] = torch.softmax(s, dim=1) @ v
    return out


def _cache(k, v, max_ctx, f16, table=None, block=0):
    kw = dict(block_table=table.data_ptr(), block_size=block, table_stride=table.shape[-1]) if table is not None else {}
    return _lib.KvCache(k=k.data_ptr(), v=v.data_ptr(), max_ctx=max_ctx, dtype=_lib.KV_F16 if f16 else _lib.KV_F32, **kw)


def _pool(kc, vc, block, seed):
    """[nkv, max_ctx, 128] (any dtype) -> pools [nb + 2, nkv, block, 128] at shuffled positions (spares: NaN), table int32"""
    nkv, max_ctx, _ = kc.shape
    nb = max_ctx // block
    ids = torch.randperm(nb + 2, generator=torch.Generator().manual_seed(seed))[:nb]
    pk = torch.full((nb + 2, nkv, block, 128), float("nan"), dtype=kc.dtype, device=kc.device)
    pv = torch.full_like(pk, float("nan"))
    for i, b in enumerate(ids.tolist()):
        pk[b] = kc[:, i * block:(i + 1) * block]
        pv[b] = vc[:, i * block:(i + 1) * block]
    return pk, pv, ids.to(torch.int32).to(kc.device)


def _unpool(pool, table):
    return torch.cat([pool[int(b)] for b in table.tolist()], dim=1)


# ------------------------------------------------------------------------------------------ writes
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("qk_norm", [False, True])
@pytest.mark.parametrize("dev_pos", [False, True])
def test_rope_kv_write_fp16_is_the_kv_round_3_cache(lib, monkeypatch, paged, qk_norm, dev_pos):
    T, nq, nkv, pos0, max_ctx, block = 70, 4, 2, 37, 256, 64
    g = torch.Generator().manual_seed(3 + paged + 2 * qk_norm)
    qkv0 = (4 * torch.randn((T, (nq + 2 * nkv) * 128), generator=g)).to(DEV)
    qn = (1 + 0.1 * torch.randn(128, generator=g)).to(DEV) if qk_norm else None
    kn = (1 + 0.1 * torch.randn(128, generator=g)).to(DEV) if qk_norm else None
    cos, sin = _rope_tables(max_ctx)
    pos_dev = torch.tensor([pos0], dtype=torch.int32, device=DEV) if dev_pos else None

    def run(f16):
        dt = torch.float16 if f16 else torch.float32
        kc = torch.full((nkv, max_ctx, 128), float("nan"), dtype=dt, device=DEV)
        vc = torch.full_like(kc, float("nan"))
        qkv = qkv0.clone()
        if paged:
            pk, pv, table = _pool(kc, vc, block, seed=5)
            c = _cache(pk, pv, max_ctx, f16, table, block)
        else:
            c = _cache(kc, vc, max_ctx, f16)
        _lib.check(lib.chatts_rope_kv_write(qkv.data_ptr(), T, nq, nkv, _lib.ptr(qn), _lib.ptr(kn), 1e-6, cos.data_ptr(), sin.data_ptr(),
                                            0 if dev_pos else pos0, _lib.ptr(pos_dev), C.byref(c), st()))
        torch.cuda.synchronize()
        if paged:
            kc, vc = _unpool(pk, table), _unpool(pv, table)
        return qkv, kc, vc

    q16, k16, v16 = run(True)
    monkeypatch.setenv("CHATTS_KV_ROUND", "3")
    q32, k32, v32 = run(False)
    assert k16.dtype == torch.float16
    assert torch.equal(q16, q32)                                             # q is rotated in place, the same bits
    assert torch.equal(k16.float()[:, pos0:pos0 + T], k32[:, pos0:pos0 + T])
    assert torch.equal(v16.float()[:, pos0:pos0 + T], v32[:, pos0:pos0 + T])
    assert torch.isnan(k16[:, :pos0]).all() and torch.isnan(v16[:, pos0 + T:]).all()     # nothing else was written


# ------------------------------------------------------------------------------------------ prefill
def _prefill_inputs(nq, nkv, T, pos0, max_ctx, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn((T, (nq + 2 * nkv) * 128), generator=g)
    k16 = torch.randn((nkv, max_ctx, 128), generator=g).half()
    v16 = torch.randn((nkv, max_ctx, 128), generator=g).half()
    k16[:, 17] *= 4
    want = _ref_attention(qkv.view(T, nq + 2 * nkv, 128)[:, :nq], k16.float(), v16.float(), pos0).numpy()
    k16[:, pos0 + T:] = float("nan")
    v16[:, pos0 + T:] = float("nan")
    return qkv.to(DEV), k16.to(DEV), v16.to(DEV), want


def _attend(lib, qkv, k, v, T, nq, nkv, pos0, max_ctx, paged, splits, wsb, seed=1):
    f16 = k.dtype == torch.float16
    if paged:
        pk, pv, table = _pool(k, v, 64, seed)
        c = _cache(pk, pv, max_ctx, f16, table, 64)
    else:
        c = _cache(k, v, max_ctx, f16)
    ws = torch.full((max(wsb, 16),), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((T, nq * 128), float("nan"), device=DEV)
    rc = lib.chatts_attention(qkv.data_ptr(), T, nq, nkv, pos0, None, C.byref(c), out.data_ptr(), splits, ws.data_ptr() if wsb else None,
                              wsb, st())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy().reshape(T, nq, 128)


@pytest.mark.parametrize("paged,nq,nkv,T,pos0", [
    (False, 10, 2, 64, 0), (False, 10, 2, 65, 31), (False, 10, 2, 130, 100), (False, 10, 2, 798, 0), (False, 5, 1, 200, 300),
    (False, 5, 1, 1000, 24), (True, 10, 2, 65, 31), (True, 10, 2, 200, 300), (True, 5, 1, 798, 0), (True, 8, 8, 130, 100)])
def test_prefill_planes_on_fp16_cache_is_bitwise_the_float32_path(lib, paged, nq, nkv, T, pos0):
    """fp16 -> bf16 hi + lo is exact: the planes, hence attn_prefill_planes_kernel's output, are those of the widened float32 cache"""
    max_ctx = 1024
    qkv, k16, v16, want = _prefill_inputs(nq, nkv, T, pos0, max_ctx, T * 7 + pos0 + nq)
    plane_bytes = ((pos0 + T + 31) // 32) * nkv * 4 * 32 * 128 * 2
    rc, o16 = _attend(lib, qkv, k16, v16, T, nq, nkv, pos0, max_ctx, paged, 1, plane_bytes)
    _lib.check(rc)
    rc, o32 = _attend(lib, qkv, k16.float(), v16.float(), T, nq, nkv, pos0, max_ctx, paged, 1, plane_bytes)
    _lib.check(rc)
    assert not np.isnan(o16).any() and np.array_equal(o16, o32)
    assert rel_err(o16, want) < 1e-5


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("nq,nkv,T,pos0,splits,path", [
    (10, 2, 70, 0, 2, "bf16x3"), (5, 1, 130, 100, 4, "bf16x3"), (8, 1, 64, 300, 1, "bf16x3"), (8, 8, 200, 31, 3, "bf16x3"),
    (10, 2, 7, 60, 1, "rows"), (5, 1, 1, 333, 16, "rows"), (4, 2, 15, 200, 4, "rows"), (8, 8, 3, 0, 1, "rows")])
def test_prefill_bf16x3_and_rows_on_fp16_cache(lib, paged, nq, nkv, T, pos0, splits, path):
    max_ctx = 512
    qkv, k16, v16, want = _prefill_inputs(nq, nkv, T, pos0, max_ctx, T + pos0 + nq + splits)
    wsb = int(lib.chatts_attn_workspace(T, nq, splits)) if splits > 1 else 0      # (bf16x3, 1 split: no workspace -> no planes)
    rc, o16 = _attend(lib, qkv, k16, v16, T, nq, nkv, pos0, max_ctx, paged, splits, wsb)
    _lib.check(rc)
    rc, o32 = _attend(lib, qkv, k16.float(), v16.float(), T, nq, nkv, pos0, max_ctx, paged, splits, wsb)
    _lib.check(rc)
    assert not np.isnan(o16).any()
    assert rel_err(o16, o32) <= 1e-6 and rel_err(o16, want) < 1e-5


def test_rows_option_on_fp16_cache(lib, monkeypatch):
    monkeypatch.setenv("CHATTS_ATTN_ROWS", "1")                             # the VALU rows kernel for every T
    nq, nkv, T, pos0, max_ctx = 10, 2, 100, 50, 512
    qkv, k16, v16, want = _prefill_inputs(nq, nkv, T, pos0, max_ctx, 11)
    rc, o16 = _attend(lib, qkv, k16, v16, T, nq, nkv, pos0, max_ctx, False, 1, 0)
    _lib.check(rc)
    rc, o32 = _attend(lib, qkv, k16.float(), v16.float(), T, nq, nkv, pos0, max_ctx, False, 1, 0)
    _lib.check(rc)
    assert rel_err(o16, o32) <= 1e-6 and rel_err(o16, want) < 1e-5


def test_float32_mfma_prefill_refuses_an_fp16_cache(lib, monkeypatch):
    monkeypatch.setenv("CHATTS_ATTN_BF16X3", "0")
    nq, nkv, T, pos0, max_ctx = 10, 2, 70, 0, 256
    qkv, k16, v16, _ = _prefill_inputs(nq, nkv, T, pos0, max_ctx, 2)
    rc, out = _attend(lib, qkv, k16, v16, T, nq, nkv, pos0, max_ctx, False, 1, 0)
    assert rc == _lib.E_BADARG and b"ATTN_BF16X3" in lib.chatts_last_error()
    assert np.isnan(out).all()                                              # refused before anything was enqueued
    rc, _ = _attend(lib, qkv, k16.float(), v16.float(), T, nq, nkv, pos0, max_ctx, False, 1, 0)
    assert rc == 0                                                          # (the float32 cache still takes that path)


# ------------------------------------------------------------------------------------------ decode
def _decode(lib, raw, k, v, pos, nq, nkv, max_ctx, splits, qn, kn, paged, block=64):
    """batched fused decode over B sequences (one [nkv, max_ctx, 128] cache each) -> (out [B, nq, 128], k, v after the call)"""
    B = raw.shape[0]
    f16 = k.dtype == torch.float16
    k, v = k.clone(), v.clone()
    cos, sin = _rope_tables(max_ctx)
    wsb = int(lib.chatts_attn_workspace(B, nq, splits))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    pos_dev = torch.tensor(pos, dtype=torch.int32, device=DEV)
    out = torch.full((B, nq * 128), float("nan"), device=DEV)
    if paged:            # one pool for all sequences, blocks interleaved
        nb = max_ctx // block
        order = torch.randperm(B * nb + 3, generator=torch.Generator().manual_seed(B + nq))[:B * nb]
        table = order.view(B, nb).to(torch.int32).to(DEV)
        pk = torch.full((B * nb + 3, nkv, block, 128), float("nan"), dtype=k.dtype, device=DEV)
        pv = torch.full_like(pk, float("nan"))
        for b in range(B):
            for i, blk in enumerate(table[b].tolist()):
                pk[blk] = k[b, :, i * block:(i + 1) * block]
                pv[blk] = v[b, :, i * block:(i + 1) * block]
        c = _cache(pk, pv, max_ctx, f16, table[0], block)
        c.table_stride = nb
        stride = 0
    else:
        c = _cache(k, v, max_ctx, f16)
        stride = nkv * max_ctx * 128
    _lib.check(lib.chatts_attention_decode_batched(raw.data_ptr(), B, nq, nkv, _lib.ptr(qn), _lib.ptr(kn), 1e-6, cos.data_ptr(),
                                                   sin.data_ptr(), 0, pos_dev.data_ptr(), C.byref(c), stride, out.data_ptr(), splits,
                                                   ws.data_ptr(), wsb, st()))
    torch.cuda.synchronize()
    if paged:
        k = torch.stack([_unpool(pk, table[b]) for b in range(B)])
        v = torch.stack([_unpool(pv, table[b]) for b in range(B)])
    return out.view(B, nq, 128).cpu(), k, v


def _rotated_q(lib, raw, pos, nq, nkv, max_ctx, qn, kn):
    """q of each sequence rotated (and normed) by chatts_rope_kv_write on a scratch cache: [B, nq, 128]"""
    cos, sin = _rope_tables(max_ctx)
    qs = []
    for b, p in enumerate(pos):
        row = raw[b:b + 1].clone()
        kc = torch.zeros((nkv, max_ctx, 128), device=DEV)
        vc = torch.zeros_like(kc)
        c = _cache(kc, vc, max_ctx, False)
        _lib.check(lib.chatts_rope_kv_write(row.data_ptr(), 1, nq, nkv, _lib.ptr(qn), _lib.ptr(kn), 1e-6, cos.data_ptr(), sin.data_ptr(),
                                            max(p, 0), None, C.byref(c), st()))
        qs.append(row.view(nq + 2 * nkv, 128)[:nq].cpu())
    torch.cuda.synchronize()
    return torch.stack(qs)


@pytest.mark.parametrize("group", [4, 5, 8])
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("splits", [1, 3, 16, 64])
def test_decode_on_fp16_cache(lib, monkeypatch, group, paged, splits):
    nkv, max_ctx = 2, 640
    nq = nkv * group
    pos = [0, 15, 16, 333, 639, -1] if not paged else [0, 63, 64, 200, 639, -1]       # tile / block edges, the last row, a parked slot
    B = len(pos)
    g = torch.Generator().manual_seed(group * 10 + splits + paged)
    raw = (2 * torch.randn((B, (nq + 2 * nkv) * 128), generator=g)).to(DEV)
    k16 = torch.randn((B, nkv, max_ctx, 128), generator=g).half()
    v16 = torch.randn((B, nkv, max_ctx, 128), generator=g).half()
    for b, p in enumerate(pos):            # fp16 NaN canaries in every row past the context (the new row at p is written first)
        k16[b, :, max(p, 0) + 1:] = float("nan")
        v16[b, :, max(p, 0) + 1:] = float("nan")
    k16, v16 = k16.to(DEV), v16.to(DEV)
    qk = group == 4
    qn = (1 + 0.1 * torch.randn(128, generator=g)).to(DEV) if qk else None
    kn = (1 + 0.1 * torch.randn(128, generator=g)).to(DEV) if qk else None
    o16, kc16, vc16 = _decode(lib, raw, k16, v16, pos, nq, nkv, max_ctx, splits, qn, kn, paged)
    monkeypatch.setenv("CHATTS_KV_ROUND", "3")
    o32, kc32, vc32 = _decode(lib, raw, k16.float(), v16.float(), pos, nq, nkv, max_ctx, splits, qn, kn, paged)
    live = [b for b, p in enumerate(pos) if p >= 0]
    for b in live:                                    # the new row: bitwise the float32 cache's under KV_ROUND=3
        p = pos[b]
        assert torch.equal(kc16[b, :, p].float(), kc32[b, :, p]) and torch.equal(vc16[b, :, p].float(), vc32[b, :, p])
    assert torch.equal(kc16[5].float().nan_to_num(7.0), k16[5].float().nan_to_num(7.0))     # the parked slot wrote nothing
    assert not torch.isnan(o16[live]).any() and (o16[5] == 0).all()
    assert rel_err(o16[live].numpy(), o32[live].numpy()) <= 1e-6
    q = _rotated_q(lib, raw, pos, nq, nkv, max_ctx, qn, kn)
    kw, vw = kc16.float().cpu(), vc16.float().cpu()
    want = torch.stack([_ref_attention(q[b:b + 1], kw[b], vw[b], pos[b])[0] for b in live]).numpy()
    assert rel_err(o16[live].numpy(), want) < 1e-5


def test_decode_fused_single_sequence_on_fp16_cache(lib, monkeypatch):
    nq, nkv, max_ctx, pos, splits = 10, 2, 512, 300, 8
    g = torch.Generator().manual_seed(5)
    raw = torch.randn((1, (nq + 2 * nkv) * 128), generator=g).to(DEV)
    k16 = torch.randn((nkv, max_ctx, 128), generator=g).half().to(DEV)
    v16 = torch.randn((nkv, max_ctx, 128), generator=g).half().to(DEV)
    k16[:, pos + 1:] = float("nan")
    v16[:, pos + 1:] = float("nan")
    cos, sin = _rope_tables(max_ctx)
    wsb = int(lib.chatts_attn_workspace(1, nq, splits))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    outs = []
    for f16 in (True, False):
        k = k16.clone() if f16 else k16.float()
        v = v16.clone() if f16 else v16.float()
        if not f16:
            monkeypatch.setenv("CHATTS_KV_ROUND", "3")
        c = _cache(k, v, max_ctx, f16)
        out = torch.full((1, nq * 128), float("nan"), device=DEV)
        _lib.check(lib.chatts_attention_decode_fused(raw.data_ptr(), nq, nkv, None, None, 1e-6, cos.data_ptr(), sin.data_ptr(), pos, None,
                                                     C.byref(c), out.data_ptr(), splits, ws.data_ptr(), wsb, st()))
        torch.cuda.synchronize()
        outs.append((out.cpu().numpy(), k[:, pos].float()))
    assert torch.equal(outs[0][1], outs[1][1])
    assert rel_err(outs[0][0], outs[1][0]) <= 1e-6


# ------------------------------------------------------------------------------------------ model
def _request(cfg, seed=0):
    from chatts_amd.processing import ChatTSProcessor
    proc = ChatTSProcessor.from_pretrained(cfg)
    rng = np.random.default_rng(seed)
    lengths = [64, 40]
    series = [random_walk_series(rng, L) for L in lengths]
    inp = proc(text=[chat_prompt(lengths)], timeseries=series, return_tensors="pt")
    return inp["input_ids"][0].tolist(), inp["timeseries"], list(lengths)


@pytest.mark.parametrize("preset", ["tiny-qwen2", "tiny-qwen3"])
@pytest.mark.parametrize("paged", [False, True])
def test_model_fp16_kv_equals_float32_model_under_kv_round_3(monkeypatch, preset, paged):
    from chatts_amd import config as cfgmod
    from chatts_amd.modeling import ChatTSForCausalLM
    cfg = cfgmod.preset(preset)
    ids, ts, lengths = _request(cfg)
    kw = dict(seed=5, max_ctx=512, max_prefill_tokens=256, kv_block_size=128 if paged else None)
    m16 = ChatTSForCausalLM.from_synthetic(cfg, kv_cache_dtype="fp16", **kw)
    assert m16.kv_cache_dtype == torch.float16 and m16.buf["kv_k"].dtype == torch.float16 and m16.buf["kv_v"].dtype == torch.float16
    toks16, lg16 = m16.generate_one(ids, ts.cuda(), lengths, 10, eos_token_id=[], return_logits=True)
    last16 = m16.buf["logits"].clone()
    graph16 = m16.graph_capturable()
    monkeypatch.setenv("CHATTS_KV_ROUND", "3")
    m32 = ChatTSForCausalLM.from_synthetic(cfg, **kw)
    assert m32.kv_cache_dtype == torch.float32
    assert m16.kv_cache_bytes_local() * 2 == m32.kv_cache_bytes_local()
    toks32, lg32 = m32.generate_one(ids, ts.cuda(), lengths, 10, eos_token_id=[], return_logits=True)
    last32 = m32.buf["logits"].clone()
    assert graph16 and m32.graph_capturable()                   # both decoded through captured graphs
    assert toks16 == toks32 and len(toks16) == 10
    assert rel_err(lg16.cpu().numpy(), lg32.cpu().numpy()) < 1e-5
    assert rel_err(last16.cpu().numpy(), last32.cpu().numpy()) < 1e-5


@pytest.mark.parametrize("paged", [False, True])
def test_continuous_batching_with_prefix_reuse_on_fp16_cache(monkeypatch, paged):
    """prefix reuse copies (contiguous: torch copy_ between slots) or adopts (paged) fp16 rows: same tokens as the KV_ROUND=3 model"""
    from chatts_amd import config as cfgmod
    from chatts_amd.modeling import ChatTSForCausalLM
    cfg = cfgmod.preset("tiny-qwen2")
    r0 = _request(cfg, 0)
    r1 = _request(cfg, 1)
    reqs = [r0, r1, r0, r0, r1]
    kw = dict(seed=5, max_ctx=512, max_prefill_tokens=256, max_batch=3, kv_block_size=64 if paged else None)
    m16 = ChatTSForCausalLM.from_synthetic(cfg, kv_cache_dtype="half", **kw)
    out16 = m16.generate_batch([(i, t.cuda(), l) for i, t, l in reqs], max_new_tokens=8, eos_token_id=None, sync_every=3)
    assert m16.prefix_stats["hits"] > 0
    monkeypatch.setenv("CHATTS_KV_ROUND", "3")
    m32 = ChatTSForCausalLM.from_synthetic(cfg, **kw)
    out32 = m32.generate_batch([(i, t.cuda(), l) for i, t, l in reqs], max_new_tokens=8, eos_token_id=None, sync_every=3)
    assert out16 == out32 and out16[0] == out16[2] == out16[3] and out16[1] == out16[4]
    # one request alone, no reuse: the same tokens as after reuse
    solo = ChatTSForCausalLM.from_synthetic(cfg, kv_cache_dtype="fp16", seed=5, max_ctx=512, max_prefill_tokens=256,
                                            enable_prefix_caching=False)
    i, t, l = r0
    assert solo.generate_one(i, t.cuda(), l, 8, eos_token_id=None) == out16[0]


def test_llm_kv_cache_dtype(monkeypatch):
    from chatts_amd import LLM, SamplingParams
    rng = np.random.default_rng(7)
    lengths = [64, 30]
    series = [random_walk_series(rng, L) for L in lengths]
    prompt = {"prompt": chat_prompt(lengths), "multi_modal_data": {"timeseries": [s.tolist() for s in series]}}
    sp = SamplingParams(max_tokens=6, ignore_eos=True)
    llm16 = LLM("tiny-qwen3", max_model_len=512, seed=3, kv_cache_dtype="fp16")
    assert llm16.model.kv_cache_dtype == torch.float16
    t16 = llm16.generate([prompt], sampling_params=sp)[0].outputs[0].token_ids
    monkeypatch.setenv("CHATTS_KV_ROUND", "3")
    llm32 = LLM("tiny-qwen3", max_model_len=512, seed=3, kv_cache_dtype="auto")
    assert llm32.model.kv_cache_dtype == torch.float32
    assert llm32.generate([prompt], sampling_params=sp)[0].outputs[0].token_ids == t16 and len(t16) == 6


def test_unknown_kv_cache_dtype_raises():
    from chatts_amd import LLM, config as cfgmod
    from chatts_amd.modeling import ChatTSForCausalLM
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        ChatTSForCausalLM.from_synthetic(cfgmod.preset("tiny-qwen2"), kv_cache_dtype="fp8", max_ctx=256, max_prefill_tokens=256)
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        LLM("tiny-qwen2", max_model_len=256, kv_cache_dtype="bf16")


TP_DRIVER = r"""
import json, sys
import numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, {root!r} + "/tests")
from chatts_amd import LLM, SamplingParams
from util import chat_prompt, random_walk_series
if __name__ == "__main__":
    llm = LLM("tiny-qwen3", tensor_parallel_size={world}, max_model_len=512, seed=3, kv_cache_dtype="fp16")
    rng = np.random.default_rng(1234)
    lengths = [64, 30]
    series = [random_walk_series(rng, L) for L in lengths]
    outs = llm.generate([{{"prompt": chat_prompt(lengths), "multi_modal_data": {{"timeseries": [s.tolist() for s in series]}}}}],
                        sampling_params=SamplingParams(max_tokens=6, ignore_eos=True))
    res = dict(dtype=str(llm.model.kv_cache_dtype), tokens=outs[0].outputs[0].token_ids)
    llm.shutdown()
    print("RESULT " + json.dumps(res), flush=True)
"""


def _run_tp(world):
    import json
    env = dict(os.environ)
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", CHATTS_FORCE_DEVICE="0", CHATTS_DIST_BACKEND="gloo", CHATTS_TP_FUSE_BLOCKS="48",
               CHATTS_TP_AR_BLOCKS="16", OMP_NUM_THREADS="8")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "CHATTS_TP_BULK_FENCE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", TP_DRIVER.format(root=ROOT, world=world)], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert lines, f"rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    return json.loads(lines[-1][7:])


def test_llm_tensor_parallel_2_fp16_kv_same_tokens_as_tp1():
    one = _run_tp(1)
    two = _run_tp(2)          # the spawned rank builds its model from the same arguments: kv_cache_dtype travels with them
    assert one["dtype"] == two["dtype"] == "torch.float16"
    assert len(one["tokens"]) == 6 and two["tokens"] == one["tokens"], (one, two)
