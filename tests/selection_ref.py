"""Float64 restatement (plain numpy) of what the selection kernels owe on ANY logits row - masked, non-finite, padded - and the
inputs of tests/test_gpu_selection_edges.py, so that tests/test_selection_ref_host.py can prove on the CPU that those inputs are fair.
TEST INFRASTRUCTURE ONLY.  The contract is written at chatts_argmax / chatts_sample_batched in include/chatts_amd.h.

A row is the slice [0, vocab) of a logits row.
  greedy       no NaN: torch.argmax (first index of the maximum; -inf allowed, the first +inf wins, all -inf -> 0).  NaN entries are
               skipped when something non-NaN exceeds -inf.  Otherwise (only NaN, or NaN and -inf): any token of the row.
  sampled      a REGULAR row (no NaN, no +inf, a finite entry) follows oracle/sampler.py; a -inf id has no mass.  A DEGENERATE row is
               selected greedily.
"""
import numpy as np

from oracle import sampler as osamp


def greedy(row):
    """-> the token (index into the row) greedy selection must return, or None where any token of the row is allowed"""
    r = np.asarray(row, dtype=np.float64)
    nan = np.isnan(r)
    if not nan.any():
        return int(np.argmax(r))                                  # first index of the maximum; an all -inf row gives 0
    r = np.where(nan, -np.inf, r)
    if (r > -np.inf).any():
        return int(np.argmax(r))
    return None


def is_degenerate(row):
    """a row the sampler must not sample from: a NaN, a +inf, or no finite entry"""
    r = np.asarray(row, dtype=np.float64)
    return bool(np.isnan(r).any() or (r == np.inf).any() or not np.isfinite(r).any())


class DrawContext:
    """What the float64 rule says about one (row, temperature, top_k, top_p): computed once, shared by every draw from that row."""

    def __init__(self, logits_row, temperature, top_k, top_p):
        self.p, self.mass = osamp.kept_set(logits_row, temperature, top_k, top_p)
        self.kept = self.p > 0
        self.pf, _ = osamp.kept_set(logits_row, temperature, 0, 1.0)
        self.cut = self.pf[self.kept].min()
        # kept set: identical unless some probability sits within rounding distance of a cut
        amb = int((np.abs(self.pf - self.cut) <= 2e-5 * self.cut).sum())
        e_rel = np.exp((np.asarray(logits_row).astype(np.float64) - np.max(logits_row)) / temperature)
        amb += int((np.abs(e_rel - osamp.MASS_FLOOR) <= 1e-4 * osamp.MASS_FLOOR).sum())     # float32 exp around the mass floor
        self.ambiguous = amb


def ambiguous(row, T, k, p):
    """How many ids could fall on either side of a cut in float32: probabilities within 2e-5 (relative) of the cut, plus exp values
    within 1e-4 (relative) of MASS_FLOOR - the count check_draw grants its n_kept / kept_mass margins by."""
    return DrawContext(row, T, k, p).ambiguous


def check_draw(logits_row, tok, temperature, top_k, top_p, seed, seq, step, n_kept, kept_mass, vocab_offset=0, ctx=None):
    """The device's choice is valid under the oracle's float64 rule (cuts and CDF boundaries get a float32 margin)."""
    c = ctx if ctx is not None else DrawContext(logits_row, temperature, top_k, top_p)
    p, pf, cut = c.p, c.pf, c.cut
    t = int(tok) - vocab_offset
    assert 0 <= t < len(p)
    assert abs(int(n_kept) - int(c.kept.sum())) <= c.ambiguous, (n_kept, c.kept.sum(), c.ambiguous)
    assert abs(float(kept_mass) - c.mass) <= 1e-4 + c.ambiguous * cut
    assert pf[t] >= cut * (1 - 2e-5), "a token outside the kept set was drawn"
    u = osamp.uniform24(seed, seq, step) / float(1 << 24)
    cum = np.cumsum(p) / p.sum()
    lo = cum[t] - p[t] / p.sum()
    assert lo - 1e-4 <= u <= cum[t] + 1e-4, (u, lo, cum[t])


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------------------
# (vocab, stride): the smallest shapes that still reach every code path of the three selection kernels
SHAPES = [(1, 4),                # one id: 15 of the sampler's 16 wave segments are empty
          (17, 20),              # seg = 2: waves 9..15 start past the end
          (1003, 1003),          # rows after the first are not 16-byte aligned: the scalar path of block_argmax_first
          (1003, 1004),          # 16-byte-aligned rows with a 3-entry scalar tail
          (4099, 4100),          # the two-launch argmax (vocab >= 4096): aligned rows, a scalar tail in the last chunk, chunks past the end
          (4099, 4101),          # ... and its scalar path: rows after the first are not 16-byte aligned
          (151936, 152064)]      # the decoder's real padded row
SAMPLER_SHAPES = [(17, 20), (1003, 1004), (4099, 4100), (151936, 152064)]
SAMPLER_STEPS = [0, 5, 123, 4000]
SAMPLER_KINDS = ("plain", "masked", "single")
VOCAB_OFFSET = 1000


def base_row(V):
    """-> (float32 Gaussian row * 2.5, the torch generator after it) - every row of a shape derives from seed V"""
    import torch
    g = torch.Generator().manual_seed(V)
    return (torch.randn(V, generator=g) * 2.5).numpy().copy(), g


def sampled_rows(V):
    """the regular rows the sampler tests draw from: {"plain", "masked" (90 % -inf, the maximum kept), "single" (one finite entry)}"""
    import torch
    base, g = base_row(V)
    mask = (torch.rand(V, generator=g) < 0.9).numpy()
    mask[int(np.argmax(base))] = False
    masked = base.copy()
    masked[mask] = -np.inf
    single = np.full(V, -np.inf, dtype=np.float32)
    single[(2 * V) // 3] = base[(2 * V) // 3]
    return {"plain": base, "masked": masked, "single": single}


def sampler_settings(V):
    """[(kind, temperature, top_k, top_p)] of the regular-row sampler test at vocabulary V"""
    common = [(1.0, 0, 1.0), (0.5, 0, 0.95), (0.7, 20, 0.9), (1.0, 50, 1.0), (1.0, 1, 1.0),
              (1e-3, 0, 1.0),              # everything but the maxima falls below the 2^-40 floor: n_kept = the number of maxima
              (50.0, 0, 1.0),              # a nearly flat row; at V = 151936 the fixed-point Z is close to 2^57
              (1.0, V - 1, 1.0), (1.0, V + 5, 1.0)]
    if V <= 4099:
        common.append((50.0, 0, 0.9))      # (at V = 151936 this setting puts 22 / 5 ids within rounding distance of the cut)
    out = [(kind, *s) for s in common for kind in SAMPLER_KINDS]
    if V == 4099:
        out.append(("masked", 1.0, 1000, 1.0))     # 384 finite entries: the 1000-th largest is -inf
    return out


def greedy_rows(V):
    """the eight rows of the greedy test, float32 [8, V]"""
    import torch
    base, g = base_row(V)
    rows = np.tile(base, (8, 1))
    mask = (torch.rand(V, generator=g) < 0.9).numpy()
    mask[int(np.argmax(base))] = False
    rows[1, mask] = -np.inf                                        # 90 % -inf
    rows[2, :] = -np.inf
    rows[2, V - 1] = base[V - 1]                                   # the only finite entry sits in the last position
    rows[3, :] = -np.inf                                           # all -inf
    rows[4, [V // 3, (2 * V) // 3]] = np.inf                       # +inf at two positions
    rows[5, V // 7] = -3.0e38                                      # the float32 extremes, denormals, and an exact tie of the maximum
    rows[5, [V // 5, V // 2]] = [1e-40, -1e-40]
    rows[5, [V // 4, (3 * V) // 4]] = 3.0e38
    nan = (torch.rand(V, generator=g) < 0.05).numpy()
    nan[[0, V - 1, int(np.argmax(base))]] = True                   # ... and the position of the maximum: skipping NaN changes the answer
    rows[6, nan] = np.nan                                          # NaN at 5 % of the positions, the first and the last among them,
    rows[7, :] = np.nan                                            # all NaN
    return rows
