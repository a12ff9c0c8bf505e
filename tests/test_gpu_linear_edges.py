"""Every path of chatts_linear, and the two RMSNorm entry points, against float64 PER ELEMENT on model-like operands.

The cases, the float64 truth (`ref64`), the componentwise scale S, the metric (`elem_err`: the worst |got - want| / S_ij) and the bars come
from tests/linear_ref.py; test_linear_ref_host.py shows on the CPU that a fault-free float32 emulation of each kernel family's documented
arithmetic passes every bar, that each of ten planted faults lands 10 x above it, and that two of them pass the norm-wise
`rel_err < 2e-5` of the older tests.  An element's bar is MARGIN * y * S_ij + 2^-23 |want_ij|, y the emulation's elem_err on the case's
own inputs - never the kernel's; the post-norm planes and chatts_rmsnorm_planes get 2^-16 |want| more (what hi + lo keeps).
tools/linear_edges.py runs the same cases through the functions of this file and writes each one's figures to profiles/linear_edges.txt.

Asserted for every element of every case: |got - want| <= bar; the output is finite (c, the plane outputs and the workspace start as
NaN: nothing may be read that the call did not write); padding columns behind a row keep their NaN; the rows of a `zero_rows` case equal
bias (+ resid) bit for bit on EPI_NONE / EPI_RESID (every path forms them as 0 + bias, then one float32 addition of the residual) and to
2^-23 max(1, |want|) behind GELU / SwiGLU.

The shape of every case was read against the dispatch code; the forced options make the choice independent of the CU count.  They are
the options the older tests set as CHATTS_<OPTION> through monkeypatch.setenv, set here for the one call by _lib.options (as
test_gpu_attention_edges.py does), so that tools/linear_edges.py can run the same functions:
  launch_gemv (M = 1, not GELU)
    gemv_ldsx_kernel<2,2,EPI,NORM>        bf16, option GEMV_KS=1 (K = 256 has one chunk: whole-K whatever GEMV_KS says)          lr.GEMV
    gemv_ksplit_kernel<EPI,NORM>          bf16, GEMV_KS 2 / 3 at K = 1600 (4 chunks) and 5120 (10): nchunks >= 4                    lr.GEMV
    gemv8_ldsx_kernel<2,2,EPI,NORM,I8>    fp8 and int8 copies (N <= 160: rows_auto = unr_auto = 2)                                  lr.GEMV
    gemv4_ldsx_kernel<2,4,EPI,NORM>       4-bit codes, groups 16 and 128 (K = 1664 for 128: the group divides K)                    lr.GEMV
  launch_gemm
    gemm_bf16x2_kernel<16 | 32 | 64 | 128, ., ., false | true>   float32 A without planes (use_stream and use_ring need planes), GEMM_BM
                                          pinned to the M-tile of M = 2 / 17 / 33 / 70 and 130, with and without the fp8 copy;
                                          GEMM_SK 1 at K = 96, 3 and 5 at K = 1056 (k / sk >= 32: honoured)                         lr.BF16X2
    gemm_stream_kernel<3 | 4 | 5, false>  planes alone, 2 <= M <= 16, K = 320 (k % 64 == 0), GEMM_STREAM_STAGES                     lr.STREAM
    gemm_stream_kernel<3 | 4, true, 1, 4 | 8>   fp8 copy, K = 384 (k % 128 == 0), GEMM_STREAM_WAVES 4 / 8                           lr.STREAM
    gemm_stream_kernel<3 | 4, true, 1, 4, true> int8 copy                                                                          lr.STREAM
    gemm_stream_kernel<4, false, 2 | 4, 4 | 8>, <3, false, 8, 4 | 8>   M = 17 / 33 / 65 and 128 at K = 1024 (stream_multiblock:
                                          k >= 1024, one 256-column panel, GEMM_STREAM_MB=128), GEMM_STREAM_MB_WAVES 4 / 8           lr.STREAM
    gemm_ring_kernel<false>               planes, GEMM_STREAM=0 (use_stream false), M >= 96 with A, M = 5 with a == NULL (use_ring:
                                          no A to fall back on); GEMM_SK 3 honoured at K = 320 / 1088 (nk / 3 >= 1), GEMM_T in range   lr.RING
    splitk_epilogue_kernel                SwiGLU behind a split, or ldc % 4 != 0                                                    lr.EPILOGUES
    splitk_epilogue_v4_kernel             every other split of the lists above, and                                                 lr.EPILOGUES
    splitk_epilogue_norm_kernel           post_norm_w, M > 16, EPI_NORM_REG=0; sk = 3, and sk = 5 (the loop over more than 4 slabs)  lr.EPILOGUES
    splitk_epilogue_norm_reg_kernel<1 | 2 | 8>  post_norm_w, M > 16, sk = 3, N = 160 / 1040 / 6160 (its = ceil(N / 1024); 7 takes <8>)  lr.EPILOGUES
    splitk_epilogue_norm_q_kernel<8, 1 | 3> post_norm_w, M <= 16, EPI_NORM_Q_GROUPS 1 / 3; sk = 2 and 5 (more than 4 slabs), N = 160 /
                                          1040 / 3088 (a row that ends inside the second batch of three column groups)               lr.EPILOGUES
  rmsnorm_kernel<false | true>            chatts_rmsnorm / chatts_rmsnorm_planes, hidden 4 and 5120                                  lr.RMSNORM
K = 1056 under GEMM_SK=3 gives gemm_bf16x2_kernel three EQUAL splits of 11 K-steps (k_per_split = 352); GEMM_SK=5 is there for the shorter
last split (224 x 4 + 160)."""
import ctypes as C
from typing import NamedTuple

import pytest
import torch

from chatts_amd import _lib
from tests import linear_ref as lr

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return _lib.load()


def st():
    return _lib.stream_ptr()


class Rec(NamedTuple):
    kernel: str
    what: str
    err: float        # elem_err of the kernel
    y: float          # the yardstick
    use: float        # the worst |got - want| / bar over the elements (and the post-norm planes): <= 1 passes
    at: tuple         # that element

    @property
    def ratio(self):
        return self.err / max(self.y, 1e-30)

    @property
    def ok(self):
        return self.use <= 1.0 and lr.MARGIN * self.y <= lr.BAR_CAP

    def line(self):
        return (f"{self.kernel:32s} {self.err:9.3g} {self.y:9.3g} {self.ratio:6.2f} {lr.MARGIN * self.y:9.3g} {self.use:6.3f} {str(self.at):12s} "
                f"{self.what}" + ("" if self.ok else "   ABOVE THE BAR"))


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _split(lib, a):
    m, k = a.shape
    hi, lo = _nan((m, k + 8), torch.bfloat16), _nan((m, k + 8), torch.bfloat16)
    _lib.check(lib.chatts_split_bf16x2(a.data_ptr(), m, k, k, hi.data_ptr(), lo.data_ptr(), k + 8, st()))
    return hi, lo


def run_linear(lib, spec, c, raw=None):
    """chatts_linear on the case under the spec's options -> (out [m, ncols], post hi + lo [m, n] float64 or None), on the host; the
    post-norm planes themselves go into `raw` (tools/linear_edges.py --digests)"""
    m, n, k, ncols = spec.m, spec.n, spec.k, spec.ncols
    ldc = ncols + spec.ldc_pad
    a, w, bias = c["a"].to(DEV), c["w"].to(DEV), c["bias"].to(DEV)
    resid = None
    if spec.epi == lr.EPI_RESID:
        resid = _nan((m, ldc))
        resid[:, :ncols] = c["resid"].to(DEV)
    out = _nan((m, ldc))
    opts = dict(spec.opts)
    if spec.family not in lr.GEMV_FAMILIES:
        opts["GEMM_SK"] = spec.sk
    with _lib.options(**opts):
        wsb = max(int(lib.chatts_linear_workspace(m, n, k)), spec.sk * m * n * 4 if spec.sk > 1 else 0)
        ws = torch.full((max(wsb, 16),), 0xFF, dtype=torch.uint8, device=DEV)          # NaN as float32
        la = _lib.LinearArgs(a=a.data_ptr(), w=w.data_ptr(), bias=bias.data_ptr(), resid=_lib.ptr(resid), c=out.data_ptr(), m=m, n=n, k=k,
                             lda=k, ldw=k, ldc=ldc, epilogue=spec.epi, workspace=ws.data_ptr(), workspace_bytes=wsb)
        if spec.norm:
            nw = c["norm_w"].to(DEV)
            la.norm_w, la.norm_eps = nw.data_ptr(), lr.EPS
        if spec.operand != "a":
            hi, lo = _split(lib, a)
            la.a_hi, la.a_lo, la.ld_planes = hi.data_ptr(), lo.data_ptr(), k + 8
            if spec.operand == "planes_only":
                la.a = None
        if spec.fmt in ("fp8", "int8"):
            q, scale = c["q"].to(DEV), c["scale"].to(DEV)
            la.w8, la.w8_scale, la.ldw8, la.w8_format = q.data_ptr(), scale.data_ptr(), k, _lib.W8_INT8 if spec.fmt == "int8" else _lib.W8_FP8
        elif spec.fmt.startswith("int4"):
            w4, sz = c["w4"].to(DEV), c["w4_sz"].to(DEV)
            la.w4, la.w4_sz, la.ldw4, la.w4_group = w4.data_ptr(), sz.data_ptr(), k // 2, c["group"]
        phi = plo = None
        if spec.post:
            pw, phi, plo = c["post_norm_w"].to(DEV), _nan((m, n + 8), torch.bfloat16), _nan((m, n + 8), torch.bfloat16)
            la.post_norm_w, la.post_norm_eps, la.post_hi, la.post_lo, la.ld_post = pw.data_ptr(), lr.EPS, phi.data_ptr(), plo.data_ptr(), n + 8
        _lib.check(lib.chatts_linear(C.byref(la), st()))
        torch.cuda.synchronize()
    out = out.cpu()
    assert torch.isnan(out[:, ncols:]).all(), spec                                     # the padding behind a row: untouched
    post = None
    if spec.post:
        phi, plo = phi.cpu(), plo.cpu()
        if raw is not None:
            raw.update(post_hi=phi[:, :n], post_lo=plo[:, :n])
        assert torch.isnan(phi[:, n:].float()).all() and torch.isnan(plo[:, n:].float()).all(), spec
        post = phi[:, :n].float().double() + plo[:, :n].float().double()
        assert torch.isfinite(post).all(), spec
    out = out[:, :ncols].contiguous()
    assert torch.isfinite(out).all(), spec
    return out, post


def check_zero_rows(spec, c, out):
    """rows 0 and m - 1 of a zero_rows case: bias (+ resid), bit for bit where that is one float32 operation"""
    for row in (0, spec.m - 1):
        if spec.epi in (lr.EPI_NONE, lr.EPI_RESID):
            want = c["bias"] + c["resid"][row] if spec.epi == lr.EPI_RESID else c["bias"]
            assert torch.equal(out[row].view(torch.int32), want.view(torch.int32)), (spec, row)
        else:
            want = c["want"][row]
            assert bool(((out[row].double() - want).abs() <= lr.U32 * want.abs().clamp_min(1.0)).all()), (spec, row)


def measure(lib, spec):
    c = lr.build(spec)
    out, post = run_linear(lib, spec, c)
    if spec.profile == "zero_rows":
        check_zero_rows(spec, c, out)
    err, _ = lr.elem_err(out, c["want"], c["S"])
    use, at = lr.bar_use(out, c["want"], c["bar"])
    if spec.post:
        use_p, at_p = lr.bar_use(post, c["want_post"], c["bar_post"])
        if use_p > use:
            use, at = use_p, ("post",) + at_p
    return Rec(spec.kernel, spec.what(), err, c["y"], use, at)


def measure_rmsnorm(lib, profile, t, hidden, seed):
    """chatts_rmsnorm and chatts_rmsnorm_planes on one case -> two Recs"""
    c = lr.rms_case(profile, t, hidden, seed)
    x, w = c["x"].to(DEV), c["w"].to(DEV)
    y = _nan((t, hidden))
    _lib.check(lib.chatts_rmsnorm(x.data_ptr(), w.data_ptr(), y.data_ptr(), t, hidden, lr.EPS, st()))
    hi, lo = _nan((t, hidden + 8), torch.bfloat16), _nan((t, hidden + 8), torch.bfloat16)
    _lib.check(lib.chatts_rmsnorm_planes(x.data_ptr(), w.data_ptr(), hi.data_ptr(), lo.data_ptr(), hidden + 8, t, hidden, lr.EPS, st()))
    torch.cuda.synchronize()
    y, hi, lo = y.cpu(), hi.cpu(), lo.cpu()
    assert torch.isfinite(y).all() and torch.isnan(hi[:, hidden:].float()).all() and torch.isnan(lo[:, hidden:].float()).all()
    planes = hi[:, :hidden].float().double() + lo[:, :hidden].float().double()
    assert torch.isfinite(planes).all()
    want, S = c["want"], c["want"].abs()
    if profile == "zero_rows":
        assert bool((y[0] == 0).all()) and bool((y[t - 1] == 0).all()) and bool((planes[0] == 0).all()) and bool((planes[t - 1] == 0).all())
    recs = []
    for kernel, got, extra in (("rmsnorm", y, 0.0), ("rmsnorm_planes", planes, lr.U_SPLIT)):
        use, at = lr.bar_use(got, want, lr.bar_of(c["y"], want, S, extra))
        recs.append(Rec(kernel, f"{profile} {t}x{hidden}", lr.elem_err(got, want, S)[0], c["y"], use, at))
    return recs


# ---- the tests ------------------------------------------------------------------------------------------------------------------------
def assert_within_bars(recs):
    """print every figure, then: no case above its bar"""
    recs = list(recs)
    for r in recs:
        print(r.line())
    over = [r.line() for r in recs if not r.ok]
    assert recs and not over, "\n" + "\n".join(over)


@pytest.mark.parametrize("fmt", ["bf16", "fp8", "int8", "int4g16", "int4g128"])
def test_gemv(lib, fmt):
    """batch 1: N 96 / 160, K half a chunk / ragged chunks / whole chunks, with and without the fused norm, EPI_NONE / RESID / SWIGLU;
    bf16 under GEMV_KS 1 / 2 / 3 (gemv_ldsx_kernel and gemv_ksplit_kernel)"""
    specs = [s for s in lr.GEMV if s.fmt == fmt]
    assert {s.norm for s in specs} == {False, True} and {s.epi for s in specs} == {lr.EPI_NONE, lr.EPI_RESID, lr.EPI_SWIGLU}
    assert_within_bars(measure(lib, s) for s in specs)


@pytest.mark.parametrize("m", [2, 17, 33, 70, 130])
def test_gemm_bf16x2(lib, m):
    """gemm_bf16x2_kernel with BM 16 / 32 / 64 / 128 on float32 A: K = 96 and K = 1056 under GEMM_SK 3 / 5, with and without the fp8 copy"""
    specs = [s for s in lr.BF16X2 if s.m == m]
    assert {s.fmt for s in specs} == {"bf16", "fp8"} and {(s.k, s.sk) for s in specs} == {(96, 1), (1056, 3), (1056, 5)}
    assert_within_bars(measure(lib, s) for s in specs)


@pytest.mark.parametrize("form", ["bf16", "fp8", "int8", "multiblock"])
def test_gemm_stream(lib, form):
    """gemm_stream_kernel on planes alone: M 2 / 7 / 16 with GEMM_SK 1 / 2 and every ring depth; 4 / 8 waves on the fp8 copy; the int8
    form; the multi-block forms at M 17 / 33 / 65 / 128"""
    specs = [s for s in lr.STREAM if (s.m > 16) == (form == "multiblock") and (form == "multiblock" or s.fmt == form)]
    assert specs and (form != "multiblock" or {s.m for s in specs} == {17, 33, 65, 128})
    assert_within_bars(measure(lib, s) for s in specs)


@pytest.mark.parametrize("m", [96, 130, 257, 5])
def test_gemm_ring(lib, m):
    """gemm_ring_kernel: N 160 / 416, K 64 / 320 / 1088, GEMM_SK 1 / 3, two GEMM_T; M = 5 on planes alone (a == NULL)"""
    specs = [s for s in lr.RING if s.m == m]
    assert {s.n for s in specs} == {160, 416} and {s.k for s in specs} >= {64, 320, 1088} and all((s.operand == "planes_only") == (m == 5) for s in specs)
    assert_within_bars(measure(lib, s) for s in specs)


def test_splitk_epilogues(lib):
    """the plain, v4 and the three post-norm split-K epilogues; under post_norm_w both c and post_hi + post_lo against their bars"""
    assert len({s.kernel for s in lr.EPILOGUES}) == 9 and any(s.post and s.profile == "wide_norm" for s in lr.EPILOGUES)
    assert_within_bars(measure(lib, s) for s in lr.EPILOGUES)


def test_rmsnorm_entry_points(lib):
    """chatts_rmsnorm and chatts_rmsnorm_planes per row on outlier / zero_rows / wide_norm, hidden 4 (the smallest accepted) and 5120"""
    assert_within_bars(r for case in lr.RMSNORM for r in measure_rmsnorm(lib, *case))
