"""Host references, yardsticks and the case lists of the linear edge tests (test_linear_ref_host.py on the CPU, test_gpu_linear_edges.py on
the GPU; tools/linear_edges.py writes the same cases' figures to profiles/linear_edges.txt).

Everything here is torch on the CPU.  The truth is `ref64` (the documented operation in float64).  A kernel's error on a case is
`elem_err`: the worst |got - want| / S over the elements, S the componentwise scale of the output (the sum of the absolute values of
everything that was added to form the element, carried through the activation's derivative), so one wrong element among thousands is
not averaged away and a product hidden under a large residual is still measured against the product's own scale.  The bar of an
element is MARGIN * y * S + 2^-23 |want|, y the elem_err of a fault-free float32 emulation of the kernel family's documented arithmetic
on the case's own inputs (`emulate`) - never of the kernel under test.  `emulate` takes named faults (FAULTS), each a failure these
kernels can really have; the host test shows that every one lands 10 x above the bar on some case of each family it applies to.

The arithmetic that `emulate` restates, from the kernels' comments:
  gemv.hip   a wave sums a row: lane l takes elements [c * chunk + l * chunk / 64, + chunk / 64) of chunk c, chunks ascending, one float32
             FMA per element with an exact product (chunk = 512 for bf16 W, 1024 for the 8-bit and 4-bit copies; x zero-padded to whole
             chunks), then the 64 lanes are added in a tree.  gemv_ksplit_kernel: wave j of ks takes the chunk pairs j, j + ks, ...,
             the waves' sums are added in wave order.  The 4-bit form meets x as a bf16 hi + lo pair in two accumulators (two products
             per step), added before the tree.  The fused RMSNorm is g * (x * rstd) in float32.
  gemm.hip / gemm_ring.hip   per output element K in ascending 32-deep blocks, the lo plane's block before the hi plane's, one float32
             accumulator; a split covers k_per_split = ceil(K / sk) rounded up to the kernel's K-step (32 register-staged, 64 ring and
             streaming, 128 streaming on an 8-bit copy), the partials are added in split order, then bias / activation / residual."""
import functools
import math
from typing import NamedTuple

import torch

from chatts_amd.modeling import pack_int4, quantize_fp8_rows, quantize_int4_rows, quantize_int8_rows

EPI_NONE, EPI_GELU, EPI_RESID, EPI_SWIGLU = 0, 1, 2, 3          # chatts_amd._lib.EPI_*
EPS = 1e-6
PROFILES = ("gauss", "outlier", "resid_stream", "cancel", "zero_rows", "wide_norm")
FAULTS = ("lo_plane_dropped", "lo_dropped_last_kstep", "last_split_short_by_one_kstep", "tail_chunk_not_zeroed", "corner_takes_neighbour_bias",
          "row_scale_of_neighbour", "int4_zero_off_by_one_group", "rstd_skips_last_chunk", "resid_row_shifted",
          "swiglu_pair_swapped_in_one_block")
MARGIN = 4.0                   # over the yardstick: one realisation of the rounding noise against another summation order (attention_ref.MARGIN)
U32 = 2.0 ** -23               # the final rounding of a float32 output and of expf, relative to the output
U_SPLIT = 2.0 ** -16           # what hi + lo keeps of a float32 value (bf16 has 8 significant bits): added to the bar of plane outputs
BAR_CAP = 2.0 ** -14           # no case may need MARGIN * y above this (the rigorous two-plane bound is 2^-16 S): choose other inputs instead
SCALED_ROW = 7                 # the 8-bit copies: this row is 37 x its neighbours, so rows 6 and 7 carry different power-of-two scales
GEMV_FAMILIES = ("gemv", "gemv8", "gemv4")
SPLIT_FAMILIES = ("bf16x2", "stream", "ring", "epi")


class Spec(NamedTuple):
    """one case: the kernel family, the label of the kernel it reaches, the operand profile, the shape and the options of the call"""
    family: str               # gemv | gemv8 | gemv4 | bf16x2 | stream | ring | epi | rmsnorm
    kernel: str               # the kernel / instantiation the dispatch code sends the call to (the profile file's first column)
    profile: str
    m: int
    n: int
    k: int
    epi: int = EPI_NONE
    fmt: str = "bf16"         # bf16 | fp8 | int8 | int4g16 | int4g128: the copy of W the call streams
    norm: bool = False        # RMSNorm of the activation fused into the prologue (M = 1)
    post: bool = False        # post_norm_w: RMSNorm(c) as planes next to c
    operand: str = "a"        # a: float32 A | planes: A and its planes | planes_only: a == NULL
    sk: int = 1               # the forced GEMM_SK (GEMV_KS for the gemv family)
    opts: tuple = ()          # further (option, value) pairs of the call
    ldc_pad: int = 0          # columns of padding behind a row of c
    seed: int = 0

    @property
    def ncols(self):
        return self.n // 2 if self.epi == EPI_SWIGLU else self.n

    def what(self):
        o = " ".join(f"{k}={v}" for k, v in self.opts)
        return (f"{self.profile} {self.m}x{self.n}x{self.k} epi={self.epi} {self.fmt}{' norm' if self.norm else ''}{' post' if self.post else ''}"
                f" {self.operand} sk={self.sk}{' ldc+' + str(self.ldc_pad) if self.ldc_pad else ''}{' ' + o if o else ''}")


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _outlier_a(g, m, k):
    """background 0.5 randn; channels 0, k - 1 and one seeded interior channel x +300, -800, +200: the first K-step, the last K-step
    (or the tail chunk), and - past the middle of K - the last split"""
    a = 0.5 * torch.randn((m, k), generator=g)
    a[:, 0] *= 300.0
    a[:, k - 1] *= -800.0
    if k > 4:
        a[:, int(torch.randint(k // 2 + 1, k - 1, (1,), generator=g))] *= 200.0
    return a


def make_case(profile, m, n, k, epi, seed, fmt="bf16"):
    """-> dict: a [m, k] float32, w [n, k] bf16 (the matrix every copy encodes), bias [n], resid [m, ncols], norm_w [k], post_norm_w [n]
    float32; for the 8-bit copies q / scale, for the 4-bit ones w4 / w4_sz / codes / qscale / qzero / group"""
    assert profile in PROFILES
    g = torch.Generator().manual_seed(seed)
    ncols = n // 2 if epi == EPI_SWIGLU else n
    w = 0.05 * torch.randn((n, k), generator=g)
    bias = torch.randn(n, generator=g)
    resid = torch.randn((m, ncols), generator=g)
    norm_w = 1 + 0.1 * torch.randn(k, generator=g)
    post_norm_w = 1 + 0.1 * torch.randn(n, generator=g)
    if profile == "gauss":                       # tests/test_gpu_kernels.py: _rand_problem
        a = torch.randn((m, k), generator=g)
    elif profile in ("outlier", "wide_norm"):
        a = _outlier_a(g, m, k)
        if profile == "wide_norm":               # norm weights log-uniform in [0.02, 20]
            norm_w = 0.02 * torch.exp(math.log(1000.0) * torch.rand(k, generator=g))
            post_norm_w = 0.02 * torch.exp(math.log(1000.0) * torch.rand(n, generator=g))
    elif profile == "resid_stream":              # o_proj / down_proj in the decoder: the residual stream far above the product
        assert epi == EPI_RESID
        a = 0.01 * torch.randn((m, k), generator=g)
        w = 0.005 * torch.randn((n, k), generator=g)
        bias = 0.01 * torch.randn(n, generator=g)
        resid = 3.0 * torch.randn((m, ncols), generator=g)
        resid[:, ::37] *= 300.0
    elif profile == "cancel":                    # a >= 0 equal on the channels of a pair, w in pairs of opposite sign: the products cancel
        assert epi == EPI_NONE and not fmt.startswith("int4")
        a = torch.randn((m, k), generator=g).abs()
        a[:, 1::2] = a[:, 0::2] * (1 + 2e-4 * torch.randn((m, k // 2), generator=g))
        bias = torch.zeros(n)
    elif profile == "zero_rows":                 # padding tokens
        a = torch.randn((m, k), generator=g)
        a[0] = 0.0
        a[m - 1] = 0.0
    w = w.to(torch.bfloat16)
    w[:, 0] = torch.linspace(-1, 1, n).to(torch.bfloat16)      # asymmetric structure: a transposed / permuted tile cannot pass
    if profile == "cancel":
        w[:, 1::2] = -w[:, 0::2]
    c = dict(a=a.float().contiguous(), bias=bias.float(), resid=resid.float(), norm_w=norm_w.float(), post_norm_w=post_norm_w.float())
    if fmt in ("fp8", "int8"):
        if n > SCALED_ROW + 1 and profile != "cancel":
            w[SCALED_ROW] *= 37.0
        c["q"], c["scale"], w = (quantize_fp8_rows if fmt == "fp8" else quantize_int8_rows)(w)
    elif fmt.startswith("int4"):
        c["group"] = int(fmt[5:])
        c["codes"], c["qscale"], c["qzero"], w = quantize_int4_rows(w, c["group"])
        c["w4"], c["w4_sz"] = pack_int4(c["codes"], c["qscale"], c["qzero"])
    c["w"] = w.contiguous()
    return c


# ---- the truth, the scale and the metric -------------------------------------------------------------------------------------------------
def _norm64(a, g, eps=EPS):
    a = a.double()
    return g.double() * (a * torch.rsqrt(a.pow(2).mean(-1, keepdim=True) + eps))


def _pairs(y):
    """[m, n] -> gate, up [m, n / 2]: the 16-row gate / up interleave of the packed SwiGLU projection"""
    v = y.view(y.shape[0], y.shape[1] // 32, 2, 16)
    return v[:, :, 0].reshape(y.shape[0], -1), v[:, :, 1].reshape(y.shape[0], -1)


def _silu(x):
    return x * torch.sigmoid(x)


def _gelu(x):
    return 0.5 * x * (1 + torch.erf(x * 0.7071067811865476))


def ref64(spec, c):
    """-> (want, S, want_post, S_post), float64.  want: the documented operation.  S: the componentwise scale of want.
    The post-norm pair is None unless spec.post."""
    a = _norm64(c["a"], c["norm_w"]) if spec.norm else c["a"].double()
    w, bias = c["w"].double(), c["bias"].double()
    pre = a @ w.t() + bias
    # an error of relative size e in every product and every addend moves the pre-activation by at most e * S_pre
    s_pre = a.abs() @ w.abs().t() + bias.abs()
    if spec.epi == EPI_NONE:
        want, S = pre, s_pre
    elif spec.epi == EPI_RESID:
        want, S = pre + c["resid"].double(), s_pre + c["resid"].double().abs()
    elif spec.epi == EPI_GELU:                  # |gelu'| <= 1.13 (its maximum, at x = sqrt(2)): |gelu(x + d) - gelu(x)| <= 1.13 |d|
        want, S = _gelu(pre), 1.13 * s_pre
    else:                                       # silu(g) u: d = silu'(g) dg u + silu(g) du, |silu'| <= 1.1
        (gate, up), (s_gate, s_up) = _pairs(pre), _pairs(s_pre)
        want, S = _silu(gate) * up, 1.1 * up.abs() * s_gate + _silu(gate).abs() * s_up
    if not spec.post:
        return want, S, None, None
    # p_j = g_j c_j r, r = rsqrt(mean c^2 + eps).  dp_j = g_j (r dc_j + c_j dr) and dr = -r^3 mean(c dc), so with |dc| <= S:
    # |dp_j| <= |g_j| r (S_j + |c_j| r^2 mean(|c| S))
    g = c["post_norm_w"].double()
    r = torch.rsqrt(want.pow(2).mean(-1, keepdim=True) + EPS)
    return want, S, g * want * r, g.abs() * r * (S + want.abs() * r * r * (want.abs() * S).mean(-1, keepdim=True))


def elem_err(got, want, S):
    """-> (max_ij |got - want| / S_ij, its index); an element whose scale is 0 must be exact"""
    d = (torch.as_tensor(got).double().reshape(want.shape) - want).abs()
    q = torch.where(S > 0, d / S.clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, math.inf)))
    q = torch.where(torch.isnan(q), torch.full_like(q, math.inf), q)
    i = int(q.argmax())
    return float(q.reshape(-1)[i]), tuple(int(x) for x in torch.unravel_index(torch.tensor(i), q.shape))


def bar_of(y, want, S, extra=0.0):
    """the bar of every element: MARGIN * y * S + (2^-23 + extra) |want|"""
    return MARGIN * y * S + (U32 + extra) * want.abs()


def bar_use(got, want, bar):
    """-> (max_ij |got - want| / bar_ij, its index): <= 1 passes"""
    return elem_err(got, want, bar)


# ---- the emulation of the documented arithmetic, with faults -----------------------------------------------------------------------------
def _fma(acc, x, y):
    """float32 fma: the product of a <= 8-bit by a 24-bit significand is exact in float64, the sum is rounded once more to float32"""
    return (acc.double() + x.double() * y.double()).float()


def _hi_lo(x):
    hi = x.to(torch.bfloat16).float()
    return hi, (x - hi).to(torch.bfloat16).float()


def chunk_of(fmt):
    return 512 if fmt == "bf16" else 1024


def kstep_of(spec):
    """the K-step k_per_split is rounded to (launch_gemm)"""
    if spec.family == "ring":
        return 64
    if spec.family in ("stream", "epi") and spec.operand != "a":
        return 128 if spec.fmt in ("fp8", "int8") and spec.m <= 16 else 64
    return 32


def split_ranges(spec):
    """[(k0, k1)] of the splits launch_gemm makes at the forced GEMM_SK (asserts that the kernel honours it)"""
    bk, k, sk = kstep_of(spec), spec.k, spec.sk
    if spec.family == "ring":
        assert sk == 1 or (k // 64) // sk >= 1 or k == 64
        if (k // 64) // sk < 1:
            sk = 1                                # K = 64: one K-step, ring_pick keeps one split
    elif bk == 32:
        assert k // sk >= 32
    else:
        assert sk <= k // bk
    kps = -(-(-(-k // sk)) // bk) * bk
    return [(k0, min(k0 + kps, k)) for k0 in range(0, k, kps)]


def _epilogue32(spec, c, acc, fault):
    """acc [m, n] float32 -> the float32 output: bias, activation / residual (gemm_store and gemv_epilogue)"""
    m, n = acc.shape
    bias = c["bias"].clone()
    v = acc + bias
    if fault == "corner_takes_neighbour_bias":
        v[m - 1, n - 1] = acc[m - 1, n - 1] + bias[n - 2]
    if spec.epi == EPI_GELU:
        return _gelu(v)
    if spec.epi == EPI_RESID:
        r = c["resid"]
        if fault == "resid_row_shifted":
            r = torch.roll(r, -1, 0) if m > 1 else torch.roll(r, -1, 1)
        return r + v
    if spec.epi == EPI_SWIGLU:
        gate, up = _pairs(v)
        out = _silu(gate) * up
        if fault == "swiglu_pair_swapped_in_one_block":
            out[:, :16] = _silu(up[:, :16]) * gate[:, :16]
        return out
    return v


def _scale_fault(spec, c, acc):
    """row_scale_of_neighbour: row j's sum scaled by row j + 1's power-of-two scale, for j = SCALED_ROW - 1"""
    if spec.fmt not in ("fp8", "int8") or spec.n <= SCALED_ROW + 1:
        return None
    j = SCALED_ROW - 1
    acc = acc.clone()
    acc[:, j] = acc[:, j] * (c["scale"][j + 1] / c["scale"][j])
    return acc


def _emulate_gemv(spec, c, fault):
    n, k, chunk = spec.n, spec.k, chunk_of(spec.fmt)
    per, nchunks = chunk // 64, -(-k // chunk)
    int4 = spec.fmt.startswith("int4")
    x = c["a"][0].clone()
    if spec.norm:
        xs = x
        if fault == "rstd_skips_last_chunk":
            if nchunks < 2:
                return None
            xs = x[:(nchunks - 1) * chunk]
        rstd = torch.rsqrt((xs * xs).sum() / torch.tensor(float(k)) + torch.tensor(EPS))
        x = c["norm_w"] * (x * rstd)
    elif fault == "rstd_skips_last_chunk":
        return None
    w = c["w"].float()
    if fault == "int4_zero_off_by_one_group":
        if not int4 or k // c["group"] < 2:
            return None
        z = torch.roll(c["qzero"], -1, 1)
        G = c["group"]
        w = (c["codes"].float().view(n, k // G, G) * c["qscale"][:, :, None] - (c["qscale"] * z)[:, :, None]).to(torch.bfloat16).float().view(n, k)
    pad = nchunks * chunk - k
    if fault == "tail_chunk_not_zeroed":         # the padding of x holds a stale 1.0 and the loads past the row's end are not masked
        if pad == 0:
            return None
        x = torch.cat([x, torch.ones(pad)])
        beyond = ((torch.arange(n)[:, None] + 1) * k + torch.arange(pad)[None, :]) % (n * k)      # what follows the row in memory
        w = torch.cat([w, w.reshape(-1)[beyond]], dim=1)
    else:
        x = torch.cat([x, torch.zeros(pad)])
        w = torch.cat([w, torch.zeros((n, pad))], dim=1)
    xv, wv = x.view(nchunks, 64, per), w.view(n, nchunks, 64, per).double()
    ks = spec.sk if spec.family == "gemv" and nchunks >= 4 else 1
    if fault in ("lo_plane_dropped", "lo_dropped_last_kstep") and not int4:
        return None
    if fault == "last_split_short_by_one_kstep":
        return None
    rnd = lambda t: t.float().double()            # noqa: E731  (one float32 rounding of a float64 value)
    if int4:
        xh, xl = (t.double() for t in _hi_lo(xv))
    else:
        xd = xv.double()
    total = None
    for j in range(ks):                           # wave j of a row group: the chunk pairs j, j + ks, ...
        mine = [ch for ch in range(nchunks) if (ch // 2) % ks == j]
        if int4:
            ah, al = torch.zeros((n, 64), dtype=torch.float64), torch.zeros((n, 64), dtype=torch.float64)
            for ch in mine:
                drop = fault == "lo_plane_dropped" or (fault == "lo_dropped_last_kstep" and ch == nchunks - 1)
                ph = (wv[:, ch] * xh[ch]).view(n, 64, per // 2, 2).sum(-1)       # v_dot2c_f32_bf16: two exact products, added exactly,
                pl = (wv[:, ch] * xl[ch]).view(n, 64, per // 2, 2).sum(-1)       # into the float32 accumulator
                for e in range(per // 2):
                    ah = rnd(ah + ph[:, :, e])
                    if not drop:
                        al = rnd(al + pl[:, :, e])
            acc = (ah + al).float()
        else:
            acc = torch.zeros((n, 64), dtype=torch.float64)
            for ch in mine:
                prod = wv[:, ch] * xd[ch]          # exact: an 8-bit by a 24-bit significand
                for e in range(per):
                    acc = rnd(acc + prod[:, :, e])   # one float32 FMA
            acc = acc.float()
        lanes = torch.arange(64)
        for o in (1, 2, 4, 8, 16, 32):            # the 64 lanes in a tree
            acc = acc + acc[:, lanes ^ o]
        total = acc[:, 0] if total is None else total + acc[:, 0]
    acc = total[None, :]
    if fault == "row_scale_of_neighbour":
        acc = _scale_fault(spec, c, acc)
        if acc is None:
            return None
    return _epilogue32(spec, c, acc, fault)


def _emulate_split(spec, c, fault):
    if fault in ("tail_chunk_not_zeroed", "int4_zero_off_by_one_group", "rstd_skips_last_chunk"):
        return None
    m, n, k = spec.m, spec.n, spec.k
    hi, lo = _hi_lo(c["a"])
    w = c["w"].float()
    nb = k // 32
    wb = w.view(n, nb, 32).permute(1, 2, 0).contiguous()                    # [nb, 32, n]
    p_hi = torch.bmm(hi.view(m, nb, 32).permute(1, 0, 2).contiguous(), wb)   # [nb, m, n]: each 32-deep block summed in float32
    p_lo = torch.bmm(lo.view(m, nb, 32).permute(1, 0, 2).contiguous(), wb)
    ranges = split_ranges(spec)
    total = None
    for si, (k0, k1) in enumerate(ranges):
        acc = torch.zeros((m, n))
        last = si == len(ranges) - 1
        b1 = k1 // 32
        if fault == "last_split_short_by_one_kstep" and last:
            b1 -= kstep_of(spec) // 32
        for b in range(k0 // 32, b1):
            drop = fault == "lo_plane_dropped" or (fault == "lo_dropped_last_kstep" and last and b >= k1 // 32 - kstep_of(spec) // 32)
            if not drop:
                acc = acc + p_lo[b]
            acc = acc + p_hi[b]
        total = acc if total is None else total + acc                       # the partials in split order
    if fault == "row_scale_of_neighbour":
        total = _scale_fault(spec, c, total)
        if total is None:
            return None
    return _epilogue32(spec, c, total, fault)


def emulate(spec, c, fault=None):
    """the float32 emulation of the family's documented arithmetic -> out [m, ncols] float32, or None when the fault does not apply to
    the case (the format, epilogue or shape has no such step)"""
    assert fault is None or fault in FAULTS
    if fault == "corner_takes_neighbour_bias" and spec.epi == EPI_SWIGLU:
        return None
    if fault == "resid_row_shifted" and spec.epi != EPI_RESID:
        return None
    if fault == "swiglu_pair_swapped_in_one_block" and spec.epi != EPI_SWIGLU:
        return None
    return (_emulate_gemv if spec.family in GEMV_FAMILIES else _emulate_split)(spec, c, fault)


def post32(spec, c, out):
    """the post-norm planes of a float32 c as the kernels form them: float32 RMSNorm, split to bf16 hi + lo -> hi + lo in float64"""
    r = torch.rsqrt((out * out).mean(-1, keepdim=True) + torch.tensor(EPS))
    hi, lo = _hi_lo(c["post_norm_w"] * (out * r))
    return hi.double() + lo.double()


# ---- rmsnorm on its own ------------------------------------------------------------------------------------------------------------------
def rms_case(profile, t, hidden, seed):
    """-> dict x [t, hidden], w [hidden], want (float64), y (the elem_err of the float32 form against S = |want|: every step is a product)"""
    g = torch.Generator().manual_seed(seed)
    w = 1 + 0.1 * torch.randn(hidden, generator=g)
    if profile == "zero_rows":
        x = 3 * torch.randn((t, hidden), generator=g)
        x[0] = 0.0
        x[t - 1] = 0.0
    else:
        x = _outlier_a(g, t, hidden)
        if profile == "wide_norm":
            w = 0.02 * torch.exp(math.log(1000.0) * torch.rand(hidden, generator=g))
    x, w = x.float(), w.float()
    want = _norm64(x, w)
    r = torch.rsqrt((x * x).mean(-1, keepdim=True) + torch.tensor(EPS))
    return dict(x=x, w=w, want=want, y=elem_err(w * (x * r), want, want.abs())[0])


# ---- a case with its truth, yardstick and bars -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def build(spec):
    c = make_case(spec.profile, spec.m, spec.n, spec.k, spec.epi, spec.seed, spec.fmt)
    c["want"], c["S"], c["want_post"], c["S_post"] = ref64(spec, c)
    c["emu"] = emulate(spec, c)
    c["y"], _ = elem_err(c["emu"], c["want"], c["S"])
    c["bar"] = bar_of(c["y"], c["want"], c["S"])
    if spec.post:
        c["bar_post"] = bar_of(c["y"], c["want_post"], c["S_post"], U_SPLIT)
    return c


# ---- the case lists (shared by the host test, the GPU test and tools/linear_edges.py) ----------------------------------------------------
def _profiles(epi, norm=False, post=False):
    out = ["gauss", "outlier"]
    if epi == EPI_RESID and not norm:           # (a normed activation has rms 1: its product cannot hide under this residual, and the
        out.append("resid_stream")              # decoder's o_proj / down_proj carry no norm)
    if norm or post:
        out.append("wide_norm")
    return out


def _gemv_cases():
    """batch 1: every format x N {96, 160} x K {half a chunk, ragged chunks, whole chunks} x (GEMV_KS 1 / 2 / 3 for bf16) x fused norm x
    every epilogue of the M = 1 path (GELU at M = 1 takes the GEMM).  K = 256 has one chunk: no K-split whatever GEMV_KS says."""
    out, i = [], 0
    for fmt, family in (("bf16", "gemv"), ("fp8", "gemv8"), ("int8", "gemv8"), ("int4g16", "gemv4"), ("int4g128", "gemv4")):
        for n in (96, 160):
            for k in (256, 1600, 5120):
                if fmt == "int4g128":
                    k = -(-k // 128) * 128      # the group divides K: 1600 -> 1664 (still ragged chunks)
                for ks in ((1, 2, 3) if fmt == "bf16" else (1,)):
                    split = fmt == "bf16" and ks > 1 and -(-k // 512) >= 4
                    if fmt == "bf16" and ks > 1 and not split:
                        continue
                    kernel = {"gemv": "gemv_ksplit" if split else "gemv_ldsx", "gemv8": f"gemv8_ldsx<{fmt}>", "gemv4": "gemv4_ldsx"}[family]
                    for norm in (False, True):
                        for epi in (EPI_NONE, EPI_RESID, EPI_SWIGLU):
                            for profile in _profiles(epi, norm):
                                out.append(Spec(family, kernel, profile, 1, n, k, epi, fmt, norm, sk=ks, opts=(("GEMV_KS", ks),) if fmt == "bf16" else (),
                                                seed=100 + i))
                                i += 1
    for fmt, family, kernel in (("bf16", "gemv", "gemv_ldsx"), ("fp8", "gemv8", "gemv8_ldsx<fp8>"), ("int4g16", "gemv4", "gemv4_ldsx")):
        opts = (("GEMV_KS", 1),) if fmt == "bf16" else ()
        for norm in (False, True):
            out.append(Spec(family, kernel, "zero_rows", 1, 160, 1600, EPI_RESID, fmt, norm, opts=opts, seed=100 + i))
            out.append(Spec(family, kernel, "zero_rows", 1, 160, 1600, EPI_SWIGLU, fmt, norm, opts=opts, seed=101 + i))
            i += 2
        if fmt != "int4g16":
            out.append(Spec(family, kernel, "cancel", 1, 160, 1600, EPI_NONE, fmt, opts=opts, seed=100 + i))
            i += 1
    out.append(Spec("gemv", "gemv_ksplit", "cancel", 1, 160, 5120, EPI_NONE, "bf16", sk=3, opts=(("GEMV_KS", 3),), seed=100 + i))
    return out


BM_OF_M = {2: 16, 17: 32, 33: 64, 70: 128, 130: 128}          # pick_geometry


def _bf16x2_cases():
    """gemm_bf16x2_kernel (float32 A, no planes): BM 16 / 32 / 64 / 128 through M, N = 160 (a ragged second 128-column tile), K = 96 (three
    K-steps, one split) and K = 1056 under GEMM_SK 3 (three splits of 11 K-steps) and 5 (224, 224, 224, 224, 160: a shorter last one);
    GEMM_BM is forced to the M-tile pick_geometry takes at K >= 512 (below it the choice depends on the CU count)"""
    out, i = [], 0
    for m in (2, 17, 33, 70, 130):
        for k, sk in ((96, 1), (1056, 3), (1056, 5)):
            for fmt in ("bf16", "fp8"):
                for epi in (EPI_NONE, EPI_GELU, EPI_RESID, EPI_SWIGLU):
                    if sk == 5 and epi in (EPI_GELU, EPI_SWIGLU):
                        continue
                    for profile in _profiles(epi):
                        out.append(Spec("bf16x2", f"gemm_bf16x2<{BM_OF_M[m]},{'fp8' if fmt == 'fp8' else 'bf16'}>", profile, m, 160, k, epi, fmt, sk=sk,
                                        opts=(("GEMM_BM", BM_OF_M[m]),), seed=2000 + i))
                        i += 1
    for m in (17, 130):
        out.append(Spec("bf16x2", f"gemm_bf16x2<{BM_OF_M[m]},bf16>", "cancel", m, 160, 1056, EPI_NONE, sk=3, opts=(("GEMM_BM", BM_OF_M[m]),), seed=2000 + i))
        out.append(Spec("bf16x2", f"gemm_bf16x2<{BM_OF_M[m]},bf16>", "zero_rows", m, 160, 1056, EPI_RESID, sk=3, opts=(("GEMM_BM", BM_OF_M[m]),), seed=2001 + i))
        out.append(Spec("bf16x2", f"gemm_bf16x2<{BM_OF_M[m]},bf16>", "zero_rows", m, 160, 96, EPI_SWIGLU, sk=1, opts=(("GEMM_BM", BM_OF_M[m]),), seed=2002 + i))
        i += 3
    return out


def _stream_cases():
    """gemm_stream_kernel on planes alone: M 2 / 7 / 16, N = 160, K = 320 (384 on the 8-bit copies: three 128-deep stages), GEMM_SK 1 / 2
    (K = 320: 192 + 128; K = 384: 256 + 128), every ring depth, 4 and 8 waves on fp8, the int8 form, and the multi-block forms"""
    out, i = [], 0
    for m in (2, 7, 16):
        for sk in (1, 2):
            for stages in (3, 4, 5):
                for epi in (EPI_NONE, EPI_GELU, EPI_RESID, EPI_SWIGLU):
                    for profile in _profiles(epi):
                        out.append(Spec("stream", f"gemm_stream<{stages},bf16>", profile, m, 160, 320, epi, operand="planes_only", sk=sk,
                                        opts=(("GEMM_STREAM_STAGES", stages),), seed=3000 + i))
                        i += 1
            for fmt, stages, waves in (("fp8", 3, 4), ("fp8", 4, 4), ("fp8", 3, 8), ("fp8", 4, 8), ("int8", 3, 4), ("int8", 4, 4)):
                for epi in (EPI_NONE, EPI_RESID, EPI_SWIGLU):
                    for profile in _profiles(epi):
                        out.append(Spec("stream", f"gemm_stream<{stages},{fmt},{waves if fmt == 'fp8' else 4}w>", profile, m, 160, 384, epi, fmt,
                                        operand="planes_only", sk=sk, opts=(("GEMM_STREAM_STAGES", stages), ("GEMM_STREAM_WAVES", waves)), seed=3000 + i))
                        i += 1
    for m, mb in ((17, 2), (33, 4), (65, 8), (128, 8)):                 # multi-block: 17 <= M <= 128, K >= 1024, bf16 W; 384 + 384 + 256
        for waves in (4, 8):
            for epi in (EPI_NONE, EPI_GELU, EPI_RESID):
                for profile in _profiles(epi):
                    out.append(Spec("stream", f"gemm_stream<MB={mb},{waves}w>", profile, m, 160, 1024, epi, operand="planes_only", sk=3,
                                    opts=(("GEMM_STREAM_MB", 128), ("GEMM_STREAM_MB_WAVES", waves)), seed=3000 + i))
                    i += 1
    for m, k, sk, kernel, opts in ((7, 320, 2, "gemm_stream<4,bf16>", ()), (33, 1024, 3, "gemm_stream<MB=4,8w>", (("GEMM_STREAM_MB", 128),))):
        out.append(Spec("stream", kernel, "cancel", m, 160, k, EPI_NONE, operand="planes_only", sk=sk, opts=opts, seed=3000 + i))
        out.append(Spec("stream", kernel, "zero_rows", m, 160, k, EPI_RESID, operand="planes_only", sk=sk, opts=opts, seed=3001 + i))
        out.append(Spec("stream", kernel, "zero_rows", m, 160, k, EPI_GELU, operand="planes_only", sk=1, opts=opts, seed=3002 + i))
        i += 3
    return out


def _ring_cases():
    """gemm_ring_kernel (option GEMM_STREAM=0 keeps the multi-block streaming form away): M 96 / 130 / 257 with A and its planes, M = 5 on
    planes alone; N 160 / 416 (one ragged panel, a ragged second one); K 64 (one K-step), 320 (128 + 128 + 64 under GEMM_SK=3), 1088 (384 +
    384 + 320); two forced GEMM_T per M (the M-tiles do not change a sum)"""
    out, i = [], 0
    for m in (96, 130, 257, 5):
        for n in (160, 416):
            for k in (64, 320, 1088):
                for sk in (1, 3):
                    if k == 64 and sk == 3:
                        continue                   # one K-step: no split to force
                    ts = (1,) if m == 5 else ((2, 4) if m == 257 else (1, 2))
                    t = ts[i % len(ts)]
                    for epi in (EPI_NONE, EPI_GELU, EPI_RESID, EPI_SWIGLU):
                        for profile in _profiles(epi):
                            out.append(Spec("ring", "gemm_ring", profile, m, n, k, epi, operand="planes_only" if m == 5 else "planes", sk=sk,
                                            opts=(("GEMM_STREAM", 0), ("GEMM_T", t)), seed=4000 + i))
                            i += 1
    for t in (2, 4):
        out.append(Spec("ring", "gemm_ring", "cancel", 257, 416, 1088, EPI_NONE, operand="planes", sk=3, opts=(("GEMM_STREAM", 0), ("GEMM_T", t)), seed=4000 + i))
        out.append(Spec("ring", "gemm_ring", "zero_rows", 257, 416, 320, EPI_RESID, operand="planes", sk=3, opts=(("GEMM_STREAM", 0), ("GEMM_T", t)), seed=4001 + i))
        out.append(Spec("ring", "gemm_ring", "zero_rows", 130, 160, 64, EPI_SWIGLU, operand="planes", sk=1, opts=(("GEMM_STREAM", 0), ("GEMM_T", t // 2)), seed=4002 + i))
        i += 3
    return out


def _epi_cases():
    """the split-K epilogues, each behind the smallest producer that reaches it: splitk_epilogue_kernel (SwiGLU, or ldc % 4 != 0),
    splitk_epilogue_v4_kernel, and with post_norm_w splitk_epilogue_norm_kernel (EPI_NORM_REG=0; sk = 3, and sk = 5: its loop over more
    than four slabs), splitk_epilogue_norm_reg_kernel<1> (N = 160), <2> (N = 1040) and <8> (N = 6160: 7 column groups, the `default` of the
    instantiation table), splitk_epilogue_norm_q_kernel<8, 1> and <8, 3> (M <= 16; sk = 2, sk = 5: more than four slabs, and N = 3088: a
    row that ends inside the second batch of three column groups).  6160 and 3088 are the smallest widths past 6 x 1024 and 3 x 1024 that
    chatts_linear accepts (N % 16 == 0): four threads hold the last column group."""
    out, i = [], 0

    def add(kernel, m, n, k, epi, sk, operand, opts=(), post=False, ldc_pad=0, profiles=None):
        nonlocal i
        for profile in profiles or _profiles(epi, post=post):
            out.append(Spec("epi", kernel, profile, m, n, k, epi, post=post, operand=operand, sk=sk, opts=opts, ldc_pad=ldc_pad, seed=5000 + i))
            i += 1
    bm = (("GEMM_BM", 32),)
    add("splitk_epilogue<swiglu>", 7, 160, 320, EPI_SWIGLU, 2, "planes_only")
    add("splitk_epilogue<swiglu>", 17, 160, 1056, EPI_SWIGLU, 3, "a", bm)
    for epi in (EPI_NONE, EPI_GELU, EPI_RESID):
        add("splitk_epilogue<ldc%4>", 17, 160, 1056, epi, 5, "a", bm, ldc_pad=2)
        add("splitk_epilogue_v4", 17, 160, 1056, epi, 5, "a", bm)
        add("splitk_epilogue_v4", 7, 160, 320, epi, 2, "planes_only")
    for epi in (EPI_NONE, EPI_RESID):
        add("splitk_epilogue_norm", 17, 160, 1056, epi, 3, "a", bm + (("EPI_NORM_REG", 0),), post=True)
        add("splitk_epilogue_norm", 130, 416, 1088, epi, 3, "planes", (("GEMM_STREAM", 0), ("EPI_NORM_REG", 0)), post=True)
        add("splitk_epilogue_norm_reg<1>", 17, 160, 1056, epi, 3, "a", bm, post=True)
        add("splitk_epilogue_norm_reg<2>", 17, 1040, 1056, epi, 3, "a", bm, post=True)
        add("splitk_epilogue_norm_q<8,1>", 7, 160, 320, epi, 2, "planes_only", (("EPI_NORM_Q_GROUPS", 1),), post=True)
        add("splitk_epilogue_norm_q<8,3>", 7, 160, 320, epi, 2, "planes_only", (("EPI_NORM_Q_GROUPS", 3),), post=True)
        add("splitk_epilogue_norm_q<8,3>", 16, 1040, 320, epi, 2, "planes_only", (("EPI_NORM_Q_GROUPS", 3),), post=True)
    add("splitk_epilogue_norm_reg<1>", 17, 160, 1056, EPI_RESID, 3, "a", bm, post=True, profiles=("zero_rows",))
    add("splitk_epilogue_norm_q<8,3>", 7, 160, 320, EPI_RESID, 2, "planes_only", (("EPI_NORM_Q_GROUPS", 3),), post=True, profiles=("zero_rows",))
    add("splitk_epilogue_v4", 17, 160, 1056, EPI_NONE, 5, "a", bm, profiles=("cancel",))
    for epi in (EPI_NONE, EPI_RESID):          # (behind the cases above: their seeds stay)
        add("splitk_epilogue_norm", 17, 160, 1056, epi, 5, "a", bm + (("EPI_NORM_REG", 0),), post=True)
        add("splitk_epilogue_norm_reg<8>", 17, 6160, 1056, epi, 3, "a", bm, post=True)
        add("splitk_epilogue_norm_q<8,3>", 7, 160, 320, epi, 5, "planes_only", (("EPI_NORM_Q_GROUPS", 3),), post=True)
        add("splitk_epilogue_norm_q<8,1>", 7, 160, 320, epi, 5, "planes_only", (("EPI_NORM_Q_GROUPS", 1),), post=True)
        add("splitk_epilogue_norm_q<8,3>", 16, 3088, 320, epi, 2, "planes_only", (("EPI_NORM_Q_GROUPS", 3),), post=True)
    return out


GEMV = _gemv_cases()
BF16X2 = _bf16x2_cases()
STREAM = _stream_cases()
RING = _ring_cases()
EPILOGUES = _epi_cases()
LISTS = {"gemv": GEMV, "bf16x2": BF16X2, "stream": STREAM, "ring": RING, "epi": EPILOGUES}
# chatts_rmsnorm / chatts_rmsnorm_planes on their own: (profile, rows, hidden, seed); 4 is the smallest hidden the entry points accept
RMSNORM = [(p, 37, h, 6000 + i * 2 + j) for i, p in enumerate(("outlier", "zero_rows", "wide_norm")) for j, h in enumerate((4, 5120))]


def fault_families(fault):
    """the Spec.family values a fault applies to"""
    return {"lo_plane_dropped": ("gemv4",) + SPLIT_FAMILIES, "lo_dropped_last_kstep": ("gemv4",) + SPLIT_FAMILIES,
            "last_split_short_by_one_kstep": SPLIT_FAMILIES, "tail_chunk_not_zeroed": GEMV_FAMILIES,
            "corner_takes_neighbour_bias": GEMV_FAMILIES + SPLIT_FAMILIES, "row_scale_of_neighbour": ("gemv8", "bf16x2", "stream"),
            "int4_zero_off_by_one_group": ("gemv4",), "rstd_skips_last_chunk": GEMV_FAMILIES, "resid_row_shifted": GEMV_FAMILIES + SPLIT_FAMILIES,
            "swiglu_pair_swapped_in_one_block": GEMV_FAMILIES + SPLIT_FAMILIES}[fault]


def all_specs():
    return [s for specs in LISTS.values() for s in specs]
