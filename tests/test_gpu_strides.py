"""GPU: the leading-dimension contract of every linear entry point and operand producer (include/chatts_amd.h).

Every matrix argument of the C-ABI carries a row stride (lda, ldw, ldc, ld_planes, ld_cplanes, ld_post, ldw8, ldw4, ld_a, ld_scale, lda8,
ldx, ldq, ...); the in-tree callers always pass the width.  Here every stride is larger than the width:
  * inputs are [rows, ld] with NaN in the pad columns - a read of the pad poisons the result;
  * outputs are [rows, ld] pre-filled with a fixed NaN bit pattern - after the call the pad must still hold it, bit for bit;
  * the strided call must give the same bits as the dense call (ld == width) with the same options: a stride must not change the
    arithmetic or its order;
  * the dense call stays inside the float64 bar its parity test already uses (tests/test_gpu_kernels.py, tests/test_gpu_f16q.py).
Pads: the smallest the entry point's alignment rule allows, then a second set in which every argument gets its own larger pad, so that no
two leading dimensions of a call coincide (a kernel that indexes one operand with another's stride cannot pass).  A refused call leaves its
outputs untouched."""
import ctypes as C

import pytest
import torch

from chatts_amd import _lib
from tests import f16q_ref
from tests.test_gpu_kernels import _ref_linear
from tests.util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"

_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.uint8: torch.uint8}
NAN_BITS = {torch.float32: 0x7FC00000, torch.bfloat16: 0x7FC0, torch.float16: 0x7E00, torch.uint8: 0x7F}   # (e4m3fn NaN for bytes)
PAD_BITS = {torch.float32: 0x7FA5A5A5, torch.bfloat16: 0x7FA5, torch.float16: 0x7DA5, torch.uint8: 0xA5}
STEP = 64                                  # the larger pads: argument i gets the minimum + STEP * (i + 1) (keeps every alignment rule)


def spread(*minimum):
    """the second pad set: a distinct larger pad per argument (a dict of pads, or a tuple of them)"""
    if len(minimum) == 1 and isinstance(minimum[0], dict):
        return {key: v + STEP * (i + 1) for i, (key, v) in enumerate(minimum[0].items())}
    return tuple(v + STEP * (i + 1) for i, v in enumerate(minimum))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return _lib.load()


def st():
    return _lib.stream_ptr()


def bits(t):
    return t.view(_INT[t.dtype])


def inp(x, ld, fill=None):
    """x [rows, width] -> [rows, ld] with NaN (or `fill` bytes) in the pad columns"""
    buf = torch.empty((x.shape[0], ld), dtype=x.dtype, device=DEV)
    bits(buf).fill_(NAN_BITS[x.dtype] if fill is None else fill)
    buf[:, :x.shape[1]] = x
    return buf


def outp(rows, ld, dtype):
    """an output buffer [rows, ld] holding PAD_BITS everywhere"""
    buf = torch.empty((rows, ld), dtype=dtype, device=DEV)
    bits(buf).fill_(PAD_BITS[dtype])
    return buf


def untouched(buf, col0=0):
    return bool((bits(buf)[:, col0:] == PAD_BITS[buf.dtype]).all())


def same(x, y):
    return torch.equal(bits(x), bits(y))


def check_outputs(strided, dense, what):
    """strided / dense: name -> (buffer, valid width).  Valid regions bit-identical, pads of the strided buffers untouched."""
    assert strided.keys() == dense.keys()
    for name, (buf, width) in strided.items():
        ref = dense[name][0]
        assert same(buf[:, :width], ref[:, :width]), f"{what}: {name} differs from the dense call"
        assert untouched(buf, width), f"{what}: {name} pad columns written"


def split_bf16(x):
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------ chatts_linear (bf16 W and its copies)
def _swiglu(y):
    """the SWIGLU epilogue on a float64 product [M, N]: gate / up rows interleaved in blocks of 16 (CHATTS_EPI_SWIGLU)"""
    m, n = y.shape
    v = y.view(m, n // 32, 2, 16)
    return (torch.nn.functional.silu(v[:, :, 0]) * v[:, :, 1]).reshape(m, n // 2)


def _problem(m, n, k, epi, seed):
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn((m, k), generator=g) * 3.0).to(DEV)
    w = (torch.randn((n, k), generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    w[:, 0] = torch.linspace(-1, 1, n).to(torch.bfloat16)            # asymmetric structure: a transposed tile cannot pass
    w[5] *= 50.0                                                     # (rows of very different scales for the 8-bit copies)
    ncols = n // 2 if epi == _lib.EPI_SWIGLU else n
    P = dict(a=a, w=w, bias=torch.randn(n, generator=g).to(DEV), resid=torch.randn((m, ncols), generator=g).to(DEV),
             norm=(1 + 0.1 * torch.randn(k, generator=g)).to(DEV), post=(1 + 0.1 * torch.randn(n, generator=g)).to(DEV))
    P["hi"], P["lo"] = split_bf16(a)
    return P


# minimum pads of chatts_linear's alignment rules (lda % 4, ldw % 8, ld_planes % 8, ldw8 % 16, ldw4 % 8; the plane path wants ldc,
# ld_cplanes % 4; post-norm ld_post % 4)
LIN_PAD = dict(a=4, w=8, c=4, planes=8, cplanes=4, post=4, w8=16, w4=8)
LIN_DENSE = {key: 0 for key in LIN_PAD}
LIN_BIG = spread(LIN_PAD)


def _linear_call(lib, P, epi, pad, *, planes_in, with_a, norm=False, alias=False, cplanes=False, post=False, copy=None, ws_delta=0):
    """one chatts_linear call with every leading dimension = width + pad[...]; returns (rc, {name: (buffer, valid width)})"""
    a, w = P["a"], P["w"]
    m, k = a.shape
    n = w.shape[0]
    ncols = n // 2 if epi == _lib.EPI_SWIGLU else n
    ldc = ncols + pad["c"]
    la = _lib.LinearArgs(m=m, n=n, k=k, epilogue=epi, lda=k + pad["a"], ldw=k + pad["w"], ldc=ldc, bias=P["bias"].data_ptr())
    keep = [inp(w, k + pad["w"])]
    la.w = keep[-1].data_ptr()
    if with_a:
        keep.append(inp(a, k + pad["a"]))
        la.a = keep[-1].data_ptr()
    if planes_in:
        keep += [inp(P["hi"], k + pad["planes"]), inp(P["lo"], k + pad["planes"])]
        la.a_hi, la.a_lo, la.ld_planes = keep[-2].data_ptr(), keep[-1].data_ptr(), k + pad["planes"]
    if norm:
        la.norm_w, la.norm_eps = P["norm"].data_ptr(), 1e-6
    outs = {}
    if cplanes:
        hi, lo = outp(m, ncols + pad["cplanes"], torch.bfloat16), outp(m, ncols + pad["cplanes"], torch.bfloat16)
        la.c_hi, la.c_lo, la.ld_cplanes = hi.data_ptr(), lo.data_ptr(), ncols + pad["cplanes"]
        outs.update(c_hi=(hi, ncols), c_lo=(lo, ncols))
    if epi == _lib.EPI_RESID:
        if alias:                                             # c aliases resid: the buffer is input and output, pad holds PAD_BITS
            r = outp(m, ldc, torch.float32)
            r[:, :ncols] = P["resid"]
        else:
            r = inp(P["resid"], ldc)
        keep.append(r)
        la.resid = r.data_ptr()
    if not cplanes:
        c = keep[-1] if alias else outp(m, ldc, torch.float32)
        la.c = c.data_ptr()
        outs["c"] = (c, ncols)
    if post:
        phi, plo = outp(m, n + pad["post"], torch.bfloat16), outp(m, n + pad["post"], torch.bfloat16)
        la.post_norm_w, la.post_norm_eps, la.post_hi, la.post_lo, la.ld_post = P["post"].data_ptr(), 1e-6, phi.data_ptr(), plo.data_ptr(), n + pad["post"]
        outs.update(post_hi=(phi, n), post_lo=(plo, n))
    if copy in ("fp8", "int8"):
        q = P[copy]
        keep.append(inp(q, k + pad["w8"], fill=0x7F))         # (int8 0x7F = 127: a read of the pad changes the result)
        la.w8, la.w8_scale, la.ldw8 = keep[-1].data_ptr(), P[copy + "_scale"].data_ptr(), k + pad["w8"]
        la.w8_format = _lib.W8_INT8 if copy == "int8" else _lib.W8_FP8
    elif copy == "int4":
        keep.append(inp(P["w4"], k // 2 + pad["w4"], fill=0xFF))   # (codes 15 | 15)
        la.w4, la.w4_sz, la.ldw4, la.w4_group = keep[-1].data_ptr(), P["w4_sz"].data_ptr(), k // 2 + pad["w4"], 128
    wsb = int(lib.chatts_linear_workspace(m, n, k))
    if wsb > 0:
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
        la.workspace, la.workspace_bytes = ws.data_ptr(), wsb + ws_delta
    rc = lib.chatts_linear(la, st())
    torch.cuda.synchronize()
    return rc, outs, wsb


# name: (m, n, k, planes in, float32 A in, options that pin the family)
FAMILIES = {
    "gemv": (1, 384, 512, False, True, {}),                       # M == 1 (EPI_GELU: the register-staged kernel with 16-row tiles)
    "gemv_norm": (1, 384, 512, False, True, {}),                  # ... with the fused RMSNorm on the input
    "stream_m7": (7, 384, 1024, True, False, {}),                 # weight-streaming kernel, M <= 16
    "stream_m24": (24, 384, 1024, True, False, {}),               # ... multi-block forms: 17..32 rows
    "stream_m48": (48, 384, 1024, True, False, {}),               # 33..64
    "stream_m100": (100, 384, 1024, True, False, {"GEMM_STREAM_MB": "128"}),     # > 64
    "ring": (130, 384, 512, True, False, {"GEMM_STREAM_MB": "0"}),                # LDS-DMA ring (prefill) kernel
    "regstaged": (40, 384, 512, False, True, {}),                 # register-staged gemm_bf16x2_kernel
}
EPIS = [_lib.EPI_NONE, _lib.EPI_GELU, _lib.EPI_RESID, _lib.EPI_SWIGLU]


def _pin(monkeypatch, opts):
    for key, v in opts.items():
        monkeypatch.setenv("CHATTS_" + key, v)


def _workspace_contract(lib, P, epi, fam_kw, what):
    """the query's exact size succeeds (checked by the caller); 16 bytes fewer must be refused with c untouched"""
    rc, outs, wsb = _linear_call(lib, P, epi, LIN_PAD, ws_delta=-16, **fam_kw)
    if wsb == 0:
        assert rc == _lib.OK, what
        return
    assert rc == _lib.E_WORKSPACE, (what, rc)
    assert all(untouched(buf) for buf, _ in outs.values()), f"{what}: a refused call wrote its output"


@pytest.mark.parametrize("family,epi", [(f, e) for f in FAMILIES for e in EPIS
                                        if not (f == "gemv_norm" and e == _lib.EPI_GELU)])   # (M == 1 GELU has no fused input RMSNorm)
def test_linear_bf16_strides(lib, monkeypatch, family, epi):
    m, n, k, planes_in, with_a, opts = FAMILIES[family]
    norm = family == "gemv_norm"
    _pin(monkeypatch, opts)
    P = _problem(m, n, k, epi, seed=m + n + k + epi)
    want = _ref_linear(P["a"], P["w"], P["bias"], P["resid"], epi, P["norm"] if norm else None)
    fam = dict(planes_in=planes_in, with_a=with_a, norm=norm)
    for sk in ((None,) if m == 1 else (None, 1, 3)):
        if sk:
            monkeypatch.setenv("CHATTS_GEMM_SK", str(sk))
        what = f"{family} epi={epi} sk={sk}"
        rc, dense, _ = _linear_call(lib, P, epi, LIN_DENSE, **fam)
        _lib.check(rc)
        c_d = dense["c"][0]
        assert not torch.isnan(c_d).any(), what
        assert rel_err(c_d.cpu().numpy(), want) < 2e-5, what
        for pad in (LIN_PAD, LIN_BIG):
            rc, s, _ = _linear_call(lib, P, epi, pad, **fam)
            _lib.check(rc)
            check_outputs(s, dense, what)
            if epi == _lib.EPI_RESID:                             # c aliasing resid (stride ldc for both)
                rc, s2, _ = _linear_call(lib, P, epi, pad, alias=True, **fam)
                _lib.check(rc)
                check_outputs(s2, dense, what + " alias")
            if m > 1:                                             # the result as bf16 hi / lo planes [M, ld_cplanes]
                rc, sp, _ = _linear_call(lib, P, epi, pad, cplanes=True, **fam)
                _lib.check(rc)
                hi, lo = split_bf16(c_d)
                check_outputs(sp, {"c_hi": (hi, 0), "c_lo": (lo, 0)}, what + " plane output")
        if sk:
            _workspace_contract(lib, P, epi, fam, what)


POST_FAMILIES = ["stream_m7", "stream_m24", "ring", "regstaged"]


@pytest.mark.parametrize("epi", [_lib.EPI_NONE, _lib.EPI_RESID])
@pytest.mark.parametrize("family", POST_FAMILIES)
def test_linear_post_norm_honours_ldc_and_ld_post(lib, monkeypatch, family, epi):
    """post_norm_*: RMSNorm of the rows of c (stride ldc) written as planes [M, ld_post] - direct (GEMM_SK=1: its own launch) and fused
    into the split-K epilogue (GEMM_SK=3: the few-row or the register form; GEMM_SK=8: the few-row or the walking form) give the dense call's
    bits, and the dense planes are chatts_rmsnorm_planes of c."""
    m, n, k, planes_in, with_a, opts = FAMILIES[family]
    _pin(monkeypatch, opts)
    P = _problem(m, n, k, epi, seed=m + k + epi + 1)
    fam = dict(planes_in=planes_in, with_a=with_a, post=True)
    want = _ref_linear(P["a"], P["w"], P["bias"], P["resid"], epi)
    for sk in (1, 3, 8):
        monkeypatch.setenv("CHATTS_GEMM_SK", str(sk))
        what = f"{family} epi={epi} sk={sk}"
        rc, dense, _ = _linear_call(lib, P, epi, LIN_DENSE, **fam)
        _lib.check(rc)
        c_d = dense["c"][0]
        assert rel_err(c_d.cpu().numpy(), want) < 2e-5, what
        hi = torch.empty((m, n), dtype=torch.bfloat16, device=DEV)
        lo = torch.empty((m, n), dtype=torch.bfloat16, device=DEV)
        _lib.check(lib.chatts_rmsnorm_planes(c_d.data_ptr(), P["post"].data_ptr(), hi.data_ptr(), lo.data_ptr(), n, m, n, 1e-6, st()))
        torch.cuda.synchronize()
        assert same(dense["post_hi"][0], hi) and same(dense["post_lo"][0], lo), what
        for pad in (LIN_PAD, LIN_BIG):
            rc, s, _ = _linear_call(lib, P, epi, pad, **fam)
            _lib.check(rc)
            check_outputs(s, dense, what)
        _workspace_contract(lib, P, epi, fam, what)


@pytest.mark.parametrize("epi", [_lib.EPI_NONE, _lib.EPI_RESID, _lib.EPI_SWIGLU])
@pytest.mark.parametrize("m", [1, 7])
@pytest.mark.parametrize("copy", ["fp8", "int8", "int4"])
def test_linear_weight_copies_honour_their_strides(lib, copy, m, epi):
    """w8 (fp8 / int8, ldw8) and w4 (ldw4, w4_group) beside w (ldw): the M == 1 GEMV streams the copy, the M <= 16 streaming kernel the
    8-bit ones (an int4 copy is ignored there).  Reference: float64 on the dequantised bf16 matrix the copy encodes."""
    from chatts_amd.modeling import pack_int4, quantize_fp8_rows, quantize_int4_rows, quantize_int8_rows
    n, k = 384, 1024
    P = _problem(m, n, k, epi, seed=m + epi + len(copy))
    if copy == "int4":
        q, sc, z, deq = quantize_int4_rows(P["w"], 128)
        P["w4"], P["w4_sz"] = pack_int4(q, sc, z)
    else:
        q, scale, deq = (quantize_fp8_rows if copy == "fp8" else quantize_int8_rows)(P["w"])
        P[copy], P[copy + "_scale"] = q, scale
    P["w"] = deq.contiguous()
    norm = m == 1
    fam = dict(planes_in=m > 1, with_a=m == 1, norm=norm, copy=copy)
    rc, dense, _ = _linear_call(lib, P, epi, LIN_DENSE, **fam)
    _lib.check(rc)
    c_d = dense["c"][0]
    assert not torch.isnan(c_d).any()
    assert rel_err(c_d.cpu().numpy(), _ref_linear(P["a"], P["w"], P["bias"], P["resid"], epi, P["norm"] if norm else None)) < 2e-5
    for pad in (LIN_PAD, LIN_BIG):
        rc, s, _ = _linear_call(lib, P, epi, pad, **fam)
        _lib.check(rc)
        check_outputs(s, dense, f"{copy} m={m} epi={epi}")


# ------------------------------------------------------------------------------------------ chatts_linear_fp8 (speed mode)
@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("bm", [128, 256])
def test_linear_fp8_strides_and_tile_forms(lib, monkeypatch, bm, order, epi):
    """lda8 / ldw8 (% 16) and ldc (no rule: + 1) with both tile heights (FP8_BM: the 256-row form is never the cost model's choice) and
    both tile orders; the dense result is the float64 product of the quantised operands (the bar of
    test_linear_fp8_speed_mode_is_the_exact_product_of_the_quantised_operands)."""
    monkeypatch.setenv("CHATTS_FP8_BM", str(bm))
    monkeypatch.setenv("CHATTS_FP8_ORDER", str(order))
    m, n, k = 300, 640, 384                                   # ragged against both tile heights and the 256-column tile
    g = torch.Generator().manual_seed(bm + order + epi)
    x = (torch.randn((m, k), generator=g) * 0.7).to(DEV)
    x[:, 0] = torch.linspace(-3, 3, m).to(DEV)
    w = (torch.randn((n, k), generator=g) * 0.05).to(DEV)
    w[:, 0] = torch.linspace(-1, 1, n).to(DEV)
    bias = torch.randn(n, generator=g).to(DEV)
    ncols = n // 2 if epi == _lib.EPI_SWIGLU else n
    resid = torch.randn((m, ncols), generator=g).to(DEV)
    q8 = torch.empty((m, k), dtype=torch.uint8, device=DEV)
    sa = torch.empty(m, dtype=torch.float32, device=DEV)
    _lib.check(lib.chatts_quantize_rows_fp8(x.data_ptr(), m, k, k, None, 0.0, q8.data_ptr(), k, sa.data_ptr(), st()))
    amax = w.abs().amax(dim=1)
    ws = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    w8 = (w * (1.0 / ws)[:, None]).to(torch.float8_e4m3fn).view(torch.uint8).contiguous()

    def run(pa, pw, pc, alias=False):
        ldc = ncols + pc
        a8b, w8b = inp(q8, k + pa), inp(w8, k + pw)
        c = outp(m, ldc, torch.float32)
        r = None
        if epi == _lib.EPI_RESID:
            r = c if alias else inp(resid, ldc)
            r[:, :ncols] = resid
        fa = _lib.LinearFp8Args(a8=a8b.data_ptr(), a_scale=sa.data_ptr(), w8=w8b.data_ptr(), w_scale=ws.data_ptr(), bias=bias.data_ptr(),
                                resid=_lib.ptr(r), c=c.data_ptr(), m=m, n=n, k=k, lda8=k + pa, ldw8=k + pw, ldc=ldc, epilogue=epi)
        _lib.check(lib.chatts_linear_fp8(C.byref(fa), st()))
        torch.cuda.synchronize()
        return {"c": (c, ncols)}

    dense = run(0, 0, 0)
    a_deq = q8.view(torch.float8_e4m3fn).double().cpu() * sa.double().cpu()[:, None]
    w_deq = w8.view(torch.float8_e4m3fn).double().cpu() * ws.double().cpu()[:, None]
    y = a_deq @ w_deq.T + bias.double().cpu()
    if epi == _lib.EPI_GELU:
        y = torch.nn.functional.gelu(y)
    elif epi == _lib.EPI_RESID:
        y = y + resid.double().cpu()
    elif epi == _lib.EPI_SWIGLU:
        y = _swiglu(y)
    c_d = dense["c"][0]
    assert not torch.isnan(c_d).any()
    assert rel_err(c_d.cpu().numpy(), y.numpy()) < 1e-4
    for pa, pw, pc in ((16, 16, 1), spread(16, 16, 1)):
        check_outputs(run(pa, pw, pc), dense, f"fp8 bm={bm} order={order} epi={epi} pad={pc}")
        if epi == _lib.EPI_RESID:
            check_outputs(run(pa, pw, pc, alias=True), dense, f"fp8 bm={bm} order={order} alias")


# ------------------------------------------------------------------------------------------ chatts_linear_f16q
F16Q_PAD = dict(a=16, w=16, sc=1, c=4, cplanes=4, csc=1, post=4, psc=1)      # ld_a, ldw % 16; ldc, ld_cplanes, ld_post % 4; scales: any
F16Q_DENSE = {key: 0 for key in F16Q_PAD}
F16Q_BIG = spread(F16Q_PAD)


def _f16q_operands(lib, m, n, k, seed, tiled):
    g = torch.Generator(device="cpu").manual_seed(seed)
    w = (torch.randn((n, k), generator=g) * 0.02).to(torch.bfloat16).to(DEV)
    a = torch.randn((m, k), generator=g).to(DEV)
    a[:, ::97] *= 8.0
    hi, lo, sc = f16q_ref.split(a)
    w16, w8, w8e = f16q_ref.weights(w)
    O = dict(a=a, w=w, hi=hi, lo=lo, sc=sc, w16=w16, w8=w8, w8e=w8e, bias=torch.randn(n, generator=g).to(DEV),
             resid=torch.randn((m, n), generator=g).to(DEV), post=(torch.rand(n, generator=g) + 0.5).to(DEV))
    if tiled:
        m16 = (m + 15) // 16 * 16
        O["thi"] = torch.zeros((m16, k), dtype=torch.float16, device=DEV)
        O["tlo"] = torch.zeros((m16, k), dtype=torch.uint8, device=DEV)
        O["tsc"] = torch.empty_like(sc)
        _lib.check(lib.chatts_split_f16q(a.data_ptr(), m, k, k, O["thi"].data_ptr(), O["tlo"].data_ptr(), O["tsc"].data_ptr(), k, k // 128, 1, st()))
        O["tw16"] = torch.empty(int(lib.chatts_tile_bf16_elems(n, k)), dtype=torch.float16, device=DEV)
        O["tw8"] = torch.empty(int(lib.chatts_tile_e4m3_bytes(n, k)), dtype=torch.uint8, device=DEV)
        _lib.check(lib.chatts_tile_bf16(w16.data_ptr(), n, k, k, O["tw16"].data_ptr(), st()))
        _lib.check(lib.chatts_tile_e4m3(w8.data_ptr(), n, k, k, O["tw8"].data_ptr(), st()))
        torch.cuda.synchronize()
        assert torch.equal(O["tsc"], sc)                  # (scales stay row-major whatever the plane layout)
    return O


def _f16q_call(lib, O, epi, pad, *, tiled=False, post=False, cplanes=False, alias=False, ws_delta=0):
    """one chatts_linear_f16q call with exactly chatts_linear_f16q_workspace(m, n, k) + ws_delta bytes (NULL when the query says 0); with
    tiled planes / weights only the row-major arrays (scales, c, resid) take a pad.  Returns (rc, {name: (buffer, valid width)}, query)"""
    m, k = O["a"].shape
    n = O["w"].shape[0]
    ncols = n // 2 if epi == _lib.EPI_SWIGLU else n
    m16 = (m + 15) // 16 * 16
    rows = m16 if tiled else m
    pa, pw = (0, 0) if tiled else (pad["a"], pad["w"])
    ldc = ncols + pad["c"]
    keep = [inp(O["tsc"] if tiled else O["sc"], k // 128 + pad["sc"], fill=0xFF)]
    qa = _lib.LinearF16qArgs(a_scale=keep[0].data_ptr(), ld_a=k + pa, ld_scale=k // 128 + pad["sc"], ldw=k + pw, w8_exp=O["w8e"].data_ptr(),
                             bias=O["bias"].data_ptr(), m=m, n=n, k=k, ldc=ldc, epilogue=epi, planes_tiled=int(tiled), w_tiled=int(tiled))
    if tiled:
        qa.a_hi, qa.a_lo8, qa.w16, qa.w8 = O["thi"].data_ptr(), O["tlo"].data_ptr(), O["tw16"].data_ptr(), O["tw8"].data_ptr()
    else:
        keep += [inp(O["hi"], k + pa), inp(O["lo"], k + pa), inp(O["w16"], k + pw), inp(O["w8"], k + pw)]
        qa.a_hi, qa.a_lo8, qa.w16, qa.w8 = (t.data_ptr() for t in keep[1:5])
    outs = {}
    if epi == _lib.EPI_RESID:
        if alias:
            r = outp(m, ldc, torch.float32)
            r[:, :ncols] = O["resid"]
        else:
            r = inp(O["resid"], ldc)
        keep.append(r)
        qa.resid = r.data_ptr()
    if cplanes:                                     # the SwiGLU result as planes (tiled: ld_cplanes == the width)
        ldp = ncols if tiled else ncols + pad["cplanes"]
        chi, clo = outp(rows, ldp, torch.float16), outp(rows, ldp, torch.uint8)
        csc = outp(m, ncols // 128 + pad["csc"], torch.uint8)
        qa.c_hi, qa.c_lo8, qa.c_scale, qa.ld_cplanes, qa.ld_cscale = chi.data_ptr(), clo.data_ptr(), csc.data_ptr(), ldp, ncols // 128 + pad["csc"]
        outs.update(c_hi=(chi, ncols), c_lo8=(clo, ncols), c_scale=(csc, ncols // 128))
    else:
        c = keep[-1] if alias else outp(m, ldc, torch.float32)
        qa.c = c.data_ptr()
        outs["c"] = (c, ncols)
    if post:
        ldp = n if tiled else n + pad["post"]
        phi, plo, psc = outp(rows, ldp, torch.float16), outp(rows, ldp, torch.uint8), outp(m, n // 128 + pad["psc"], torch.uint8)
        qa.post_norm_w, qa.post_norm_eps = O["post"].data_ptr(), 1e-6
        qa.post_hi, qa.post_lo8, qa.post_scale, qa.ld_post, qa.ld_pscale = phi.data_ptr(), plo.data_ptr(), psc.data_ptr(), ldp, n // 128 + pad["psc"]
        outs.update(post_hi=(phi, n), post_lo8=(plo, n), post_scale=(psc, n // 128))
    wsb = int(lib.chatts_linear_f16q_workspace(m, n, k))
    if wsb > 0:
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
        qa.workspace, qa.workspace_bytes = ws.data_ptr(), wsb + ws_delta
    rc = lib.chatts_linear_f16q(qa, st())
    torch.cuda.synchronize()
    return rc, outs, wsb


def _f16q_refs(O, epi):
    """(float64 product of the dequantised operands, float64 true product), epilogue applied"""
    m, n = O["a"].shape[0], O["w"].shape[0]
    ref = f16q_ref.gemm(O["hi"], O["lo"], O["sc"], O["w16"], O["w8"], O["w8e"]) + O["bias"].double()
    true = O["a"].double() @ O["w"].double().t() + O["bias"].double()
    if epi == _lib.EPI_GELU:
        ref, true = torch.nn.functional.gelu(ref), torch.nn.functional.gelu(true)
    elif epi == _lib.EPI_RESID:
        ref, true = ref + O["resid"].double(), true + O["resid"].double()
    elif epi == _lib.EPI_SWIGLU:
        ref, true = _swiglu(ref), _swiglu(true)
    return ref.cpu().numpy(), true.cpu().numpy()


def _f16q_post_ref(lib, c, post_w):
    """the post-norm planes a call must write for its float32 result c: the f16q split of chatts_rmsnorm(c)"""
    m, n = c.shape
    y = torch.empty_like(c)
    _lib.check(lib.chatts_rmsnorm(c.data_ptr(), post_w.data_ptr(), y.data_ptr(), m, n, 1e-6, st()))
    torch.cuda.synchronize()
    return f16q_ref.split(y)


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("tiled", [False, True])
def test_linear_f16q_strides(lib, monkeypatch, tiled, epi):
    """ld_a / ldw / ld_scale / ldc / ld_cplanes / ld_cscale / ld_post / ld_pscale, direct (GEMM_SK=1) and split-K (GEMM_SK=2, where the
    epilogue allows a split); tiled planes / weights fix their own leading dimensions, the scales and c keep theirs."""
    m, n, k = 130, 512, 512
    O = _f16q_operands(lib, m, n, k, seed=m + epi + 7 * tiled, tiled=tiled)
    ref, true = _f16q_refs(O, epi)
    post = epi in (_lib.EPI_NONE, _lib.EPI_RESID)
    for sk in (1, 2):
        monkeypatch.setenv("CHATTS_GEMM_SK", str(sk))
        what = f"f16q tiled={tiled} epi={epi} sk={sk}"
        rc, dense, _ = _f16q_call(lib, O, epi, F16Q_DENSE, tiled=tiled, post=post)
        _lib.check(rc)
        c_d = dense["c"][0]
        assert not torch.isnan(c_d).any(), what
        assert rel_err(c_d.cpu().numpy(), ref) < 2e-6, what
        assert rel_err(c_d.cpu().numpy(), true) < 3e-5, what
        if post and not tiled:                      # the planes are chatts_rmsnorm_f16q of c
            eh, eq, es = _f16q_post_ref(lib, c_d, O["post"])
            assert same(dense["post_hi"][0], eh) and same(dense["post_lo8"][0], eq) and same(dense["post_scale"][0], es), what
        for pad in (F16Q_PAD, F16Q_BIG):
            rc, s, _ = _f16q_call(lib, O, epi, pad, tiled=tiled, post=post)
            _lib.check(rc)
            check_outputs(s, dense, what)
            if epi == _lib.EPI_RESID:
                rc, s2, _ = _f16q_call(lib, O, epi, pad, tiled=tiled, post=post, alias=True)
                _lib.check(rc)
                check_outputs(s2, dense, what + " alias")
            if epi == _lib.EPI_SWIGLU:
                rc, sp, _ = _f16q_call(lib, O, epi, pad, tiled=tiled, cplanes=True)
                _lib.check(rc)
                rc, dp, _ = _f16q_call(lib, O, epi, F16Q_DENSE, tiled=tiled, cplanes=True)
                _lib.check(rc)
                check_outputs(sp, dp, what + " plane output")
                if not tiled:
                    eh, eq, es = f16q_ref.split(c_d)
                    assert same(dp["c_hi"][0], eh) and same(dp["c_lo8"][0], eq) and same(dp["c_scale"][0], es), what


def test_linear_f16q_refuses_bad_post_planes_before_any_work(lib, monkeypatch):
    """a post-norm argument the call cannot honour is refused up front, on the direct and on the split-K path: c stays untouched"""
    m, n, k = 130, 512, 512
    O = _f16q_operands(lib, m, n, k, seed=3, tiled=False)
    for sk in ("1", "2"):
        monkeypatch.setenv("CHATTS_GEMM_SK", sk)
        rc, outs, _ = _f16q_call(lib, O, _lib.EPI_NONE, dict(F16Q_PAD, post=-4), post=True)     # ld_post = N - 4 < N
        assert rc == _lib.E_SHAPE, (sk, rc)
        assert all(untouched(buf) for buf, _ in outs.values()), sk


# ------------------------------------------------------------------------------------------ operand producers
def test_split_bf16x2_strides(lib):
    m, k = 37, 320
    g = torch.Generator().manual_seed(3)
    x = (torch.randn((m, k), generator=g) * torch.logspace(-20, 20, k)).to(DEV)
    want_hi, want_lo = split_bf16(x)
    for px, pp in ((4, 8), spread(4, 8)):
        xb = inp(x, k + px)
        hi, lo = outp(m, k + pp, torch.bfloat16), outp(m, k + pp, torch.bfloat16)
        _lib.check(lib.chatts_split_bf16x2(xb.data_ptr(), m, k, k + px, hi.data_ptr(), lo.data_ptr(), k + pp, st()))
        torch.cuda.synchronize()
        check_outputs({"hi": (hi, k), "lo": (lo, k)}, {"hi": (want_hi, k), "lo": (want_lo, k)}, f"split_bf16x2 pad={px}")


def test_split_f16q_strides(lib):
    m, k = 37, 640
    g = torch.Generator().manual_seed(4)
    x = torch.randn((m, k), generator=g).to(DEV)
    x[:, ::97] *= 8.0
    rh, rq, rs = f16q_ref.split(x)
    for px, pp, ps in ((4, 16, 1), spread(4, 16, 1)):
        xb = inp(x, k + px)
        hi, lo, sc = outp(m, k + pp, torch.float16), outp(m, k + pp, torch.uint8), outp(m, k // 128 + ps, torch.uint8)
        _lib.check(lib.chatts_split_f16q(xb.data_ptr(), m, k, k + px, hi.data_ptr(), lo.data_ptr(), sc.data_ptr(), k + pp, k // 128 + ps, 0, st()))
        torch.cuda.synchronize()
        check_outputs({"hi": (hi, k), "lo8": (lo, k), "scale": (sc, k // 128)},
                      {"hi": (rh, k), "lo8": (rq, k), "scale": (rs, k // 128)}, f"split_f16q pad={px}")


@pytest.mark.parametrize("norm", [False, True])
def test_quantize_rows_fp8_strides(lib, norm):
    """ldx / ldq: strided == dense bit for bit.  Against the restatement: without the norm every row's codes are exactly e4m3_rne(x * r)
    for r = the float32 reciprocal of the row's scale - the kernel forms 1 / scale and amax / 448 with the device's float32 division, which
    may differ from the correctly rounded one by an ulp, so the scale is held to 3e-7 and r may be either neighbour of 1 / scale (one r per
    row, every code of the row).  With the fused RMSNorm the sum of squares is a block reduction in the device's order and rsqrtf is the
    device's: that restatement is not bit-exact, and its bar lives in test_quantize_rows_fp8_fuses_rmsnorm."""
    m, k = 37, 640
    g = torch.Generator().manual_seed(5)
    x = torch.randn((m, k), generator=g).to(DEV)
    x[5] = 0.0
    nw = (1 + 0.1 * torch.randn(k, generator=g)).to(DEV) if norm else None

    def run(px, pq):
        xb = inp(x, k + px)
        q, s = outp(m, k + pq, torch.uint8), outp(1, m, torch.float32)
        _lib.check(lib.chatts_quantize_rows_fp8(xb.data_ptr(), m, k, k + px, _lib.ptr(nw), 1e-6, q.data_ptr(), k + pq, s.data_ptr(), st()))
        torch.cuda.synchronize()
        return {"q": (q, k), "scale": (s, m)}

    dense = run(0, 0)
    q, sa = dense["q"][0], dense["scale"][0][0]
    xf = x if nw is None else nw[None] * (x * torch.rsqrt((x.double() ** 2).mean(dim=1, keepdim=True) + 1e-6).float())
    amax = xf.abs().amax(dim=1)
    assert torch.allclose(sa, torch.where(amax > 0, amax / 448.0, torch.ones_like(amax)), rtol=3e-7 if nw is None else 1e-6, atol=0)
    if nw is None:
        r = 1.0 / sa
        explained = torch.zeros(m, dtype=torch.bool, device=DEV)
        for cand in (r, torch.nextafter(r, torch.full_like(r, float("inf"))), torch.nextafter(r, torch.zeros_like(r))):
            codes = (x * cand[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
            explained |= (codes == q[:, :k]).all(dim=1)
        assert explained.all(), (~explained).nonzero().flatten().tolist()
    for px, pq in ((4, 4), spread(4, 4)):
        check_outputs(run(px, pq), dense, f"quantize_rows_fp8 norm={norm} pad={px}")


def test_rmsnorm_planes_and_f16q_strides(lib):
    t, h = 37, 1280
    g = torch.Generator().manual_seed(6)
    x = (torch.randn((t, h), generator=g) * 3).to(DEV)
    w = (1 + 0.1 * torch.randn(h, generator=g)).to(DEV)
    y = torch.empty_like(x)
    _lib.check(lib.chatts_rmsnorm(x.data_ptr(), w.data_ptr(), y.data_ptr(), t, h, 1e-6, st()))
    torch.cuda.synchronize()
    want_hi, want_lo = split_bf16(y)
    eh, eq, es = f16q_ref.split(y)
    for pp, ps in ((4, 1), spread(4, 1)):
        hi, lo = outp(t, h + pp, torch.bfloat16), outp(t, h + pp, torch.bfloat16)
        _lib.check(lib.chatts_rmsnorm_planes(x.data_ptr(), w.data_ptr(), hi.data_ptr(), lo.data_ptr(), h + pp, t, h, 1e-6, st()))
        qh, ql, qs = outp(t, h + pp, torch.float16), outp(t, h + pp, torch.uint8), outp(t, h // 128 + ps, torch.uint8)
        _lib.check(lib.chatts_rmsnorm_f16q(x.data_ptr(), w.data_ptr(), qh.data_ptr(), ql.data_ptr(), qs.data_ptr(), h + pp, h // 128 + ps, t, h,
                                           1e-6, 0, st()))
        torch.cuda.synchronize()
        check_outputs({"hi": (hi, h), "lo": (lo, h)}, {"hi": (want_hi, h), "lo": (want_lo, h)}, f"rmsnorm_planes pad={pp}")
        check_outputs({"hi": (qh, h), "lo8": (ql, h), "scale": (qs, h // 128)},
                      {"hi": (eh, h), "lo8": (eq, h), "scale": (es, h // 128)}, f"rmsnorm_f16q pad={pp}")
