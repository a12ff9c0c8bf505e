"""GPU: the logit controls (csrc/logit_controls.hip) at kernel level, through the stand-alone entry points: penalised logits against the
float64 reference of tests/logit_controls_ref.py within a derived bound, the min_p survivor set, the per-sequence state, determinism
and graph replay.  The model, engine, LLM, server and tensor parallelism: tests/test_gpu_logit_controls_e2e.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from chatts_amd import _lib
from tests import logit_controls_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROMPT_BIT = 1 << 30
SEED = 20261016            # logits / state of every case below; test_min_p_... asserts that the reference alone has no id inside the band

# per-row settings of the batch-16 cases: (r, f, p, min_p, T).  Row 5 is all-default; rows 3 and 9 are greedy rows with min_p set (inert).
# (min_p = 1 puts the maximum itself on the cut, i.e. inside the band by construction: it has a test of its own)
ROWS16 = [(1.3, 0.5, 0.5, 0.0, 0.0), (1.0, 0.0, 0.0, 0.2, 0.8), (2.0, -1.0, 0.25, 0.05, 1.0), (1.1, 2.0, -2.0, 0.3, 0.0),
          (0.5, 0.0, 0.0, 0.0, 0.7), (1.0, 0.0, 0.0, 0.0, 0.0), (1.05, 0.0, 0.0, 0.999, 1.0), (1.0, 1.5, 0.0, 0.5, 0.3),
          (1.0, 0.0, 1.0, 1e-3, 1.5), (3.0, 0.1, 0.1, 0.9, 0.0), (1.3, 0.5, 0.5, 0.1, 0.2), (0.8, -0.5, -0.5, 0.6, 2.0),
          (1.0, 0.0, 0.0, 0.7, 0.5), (1.7, 0.0, 2.0, 0.0, 1.0), (1.0, -2.0, 2.0, 0.02, 0.9), (1.2, 0.3, 0.0, 0.4, 1.0)]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _case(batch, V, vocab_offset, seed=SEED):
    """float32 logits, and per row a prompt (global ids, some outside the slice) and a history with repeats (a count of 3 among them)"""
    rng = np.random.default_rng([seed, batch, V])
    x = (rng.standard_normal((batch, V)) * 3.0).astype(np.float32)
    prompts, hists = [], []
    for b in range(batch):
        prompts.append((vocab_offset - 50 + rng.integers(0, V + 100, 300)).tolist())
        h = (vocab_offset + rng.integers(0, V, 30)).tolist()
        h += [h[0]] * 2 + [h[1]] + [int(prompts[b][7])] + [vocab_offset + int(np.argmax(x[b]))] * 2      # c = 3, c = 2, a prompt id, the maximum
        hists.append(h)
    return x, prompts, hists


def _state(prompts, hists, V, vocab_offset):
    st = np.zeros((len(prompts), V), dtype=np.int32)
    for b, (p, h) in enumerate(zip(prompts, hists)):
        st[b] = ref.counts_of(h, V, vocab_offset) + PROMPT_BIT * ref.prompt_mask(p, V, vocab_offset)
    return st


def _apply(lib, x, state, rows, vocab_offset=0, graph=False, runs=1):
    """-> (out [batch, V] float32 numpy per run, the logits buffer after the pass)"""
    b, V = x.shape
    lg = torch.from_numpy(x).to(DEV)
    st = torch.from_numpy(state).to(DEV)
    out = torch.full((b, V), 7.0, device=DEV)
    par = [torch.tensor([r[i] for r in rows], dtype=torch.float32, device=DEV) for i in range(5)]
    ws = torch.zeros(int(lib.chatts_logit_controls_workspace(b)), dtype=torch.uint8, device=DEV)
    args = _lib.LogitControlArgs(state=st.data_ptr(), state_stride=V, out=out.data_ptr(), out_stride=V, repetition_rows=par[0].data_ptr(),
                                 frequency_rows=par[1].data_ptr(), presence_rows=par[2].data_ptr(), min_p_rows=par[3].data_ptr(),
                                 temperature_rows=par[4].data_ptr())

    def call():
        _lib.check(lib.chatts_logit_controls_apply(lg.data_ptr(), b, V, V, vocab_offset, C.byref(args), ws.data_ptr(), ws.numel(), _st()))
    outs = []
    if graph:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        for _ in range(runs):
            out.fill_(7.0)
            g.replay()
            torch.cuda.synchronize()
            outs.append(out.cpu().numpy())
    else:
        for _ in range(runs):
            out.fill_(7.0)
            call()
            torch.cuda.synchronize()
            outs.append(out.cpu().numpy())
    return outs, lg.cpu().numpy()


def _check_rows(x, prompts, hists, rows, got, vocab_offset):
    """penalties within the derived bound, untouched ids bit-identical, min_p survivors = the reference's outside the band.
    -> (ids inside the band in the reference alone, the worst penalty error over its bound)"""
    b, V = x.shape
    ambiguous_total, worst = 0, 0.0
    for i in range(b):
        r, f, p, mp, T = rows[i]
        cnt = ref.counts_of(hists[i], V, vocab_offset)
        inp = ref.prompt_mask(prompts[i], V, vocab_offset)
        pen = ref.penalise(x[i], inp, cnt, r, f, p)
        bound = ref.penalty_bound(x[i], cnt, r, f, p)
        cut = ref.min_p_cut(pen, T, mp)
        alive_ref = np.ones(V, bool) if cut is None else pen >= cut
        alive = got[i] != -np.inf
        if cut is None:
            assert alive.all(), i
            amb = np.zeros(V, bool)
        else:
            band = bound + bound[int(np.argmax(pen))] + 4 * ref.EPS * abs(T * np.log(mp))
            amb = np.abs(pen - cut) <= band
            print(f"row {i}: min_p {mp} T {T}: {int(alive_ref.sum())} survivors, {int(amb.sum())} ids inside the band, "
                  f"{int((alive != alive_ref).sum())} differ from the reference")
            assert not (alive != alive_ref)[~amb].any(), (i, np.nonzero((alive != alive_ref) & ~amb)[0][:8])
            assert amb.sum() <= V / 10000, (i, int(amb.sum()))
        ambiguous_total += int(amb.sum())
        seen = inp | (cnt > 0)
        same = got[i].view(np.uint32) == x[i].view(np.uint32)
        assert same[alive & ~seen].all(), i                       # ids outside prompt and history: the raw bits
        if (r, f, p) == (1.0, 0.0, 0.0):
            assert same[alive].all(), i                           # ... and every id of a row without penalties
        err = np.abs(got[i][alive].astype(np.float64) - pen[alive])
        over = err / np.maximum(bound[alive], 1e-300)
        k = seen[alive]
        if k.any():
            worst = max(worst, float(over[k].max()))
        assert (err <= bound[alive]).all(), (i, float(err.max()))
    return ambiguous_total, worst


@pytest.mark.parametrize("V,vocab_offset", [(151936, 0), (151937, 0), (4099, 0), (37984, 3 * 37984), (19009, 19009)])
@pytest.mark.parametrize("batch", [1, 16])
def test_penalties_and_min_p_match_the_float64_reference(lib, V, vocab_offset, batch):
    """|kernel - float64 reference| <= 4 * 2**-24 * (|l| * max(r, 1/r) + |f| * c + |p|) on penalised ids: at most four float32 roundings,
    each at most half an ulp of a magnitude bounded by that sum (whether or not the compiler contracts the multiply-subtract).  min_p: the
    survivor set is the reference's, except ids whose reference distance from the cut is inside the band (their bound + the row
    maximum's + 4 * 2**-24 * |T log min_p| for the float32 logarithm and product); SEED is one for which the reference has none."""
    rows = ROWS16[:batch] if batch > 1 else [ROWS16[2]]
    x, prompts, hists = _case(batch, V, vocab_offset)
    state = _state(prompts, hists, V, vocab_offset)
    (got,), after = _apply(lib, x, state, rows, vocab_offset)
    assert np.array_equal(after.view(np.uint32), x.view(np.uint32))              # the raw logits are only read
    ambiguous, worst = _check_rows(x, prompts, hists, rows, got, vocab_offset)
    print(f"V={V} batch={batch}: worst penalty error {worst:.3f} of its bound; {ambiguous} ids inside a min_p band")
    assert ambiguous == 0                                                         # (a property of SEED, checked on the CPU when it was chosen)


def test_min_p_one_keeps_exactly_the_maxima_and_ties_at_the_cut(lib):
    V = 151936
    x, prompts, hists = _case(2, V, 0)
    x[0, [5, 70000, 151935]] = 40.0                                               # three maxima
    x[1, 9] = 16.0                                                                # the maximum of row 1
    state = np.zeros((2, V), dtype=np.int32)
    rows = [(1.0, 0.0, 0.0, 1.0, 0.6), (1.0, 0.0, 0.0, 0.0, 0.0)]
    (got,), _ = _apply(lib, x, state, rows)
    assert np.nonzero(got[0] != -np.inf)[0].tolist() == [5, 70000, 151935] and (got[0][[5, 70000, 151935]] == 40.0).all()
    assert np.array_equal(got[1].view(np.uint32), x[1].view(np.uint32))
    # a tie at the cut is kept: float32 logf(0.25) * 4 is within an ulp of -8 log 2; put two ids exactly on the kernel's own cut
    cut = np.float32(16.0) + np.float32(4.0) * np.log(np.float32(0.25))
    for c in (np.nextafter(cut, np.float32(np.inf)), cut, np.nextafter(cut, np.float32(-np.inf))):
        x[1, [100, 2000]] = c
        (g2,), _ = _apply(lib, x, state, [rows[0], (1.0, 0.0, 0.0, 0.25, 4.0)])
        alive = g2[1, [100, 2000]] != -np.inf
        assert alive[0] == alive[1]                                               # equal logits share their fate, whatever the last bit of the cut
    x[1, [100, 2000]] = np.float32(16.0) - np.float32(5.0)                        # clearly above the cut (16 - 5.545)
    (g3,), _ = _apply(lib, x, state, [rows[0], (1.0, 0.0, 0.0, 0.25, 4.0)])
    assert (g3[1, [100, 2000]] == np.float32(11.0)).all() and g3[1, 9] == 16.0


def test_state_reset_mark_and_update(lib):
    V, off, n = 19009, 1000, 4
    rng = np.random.default_rng(SEED)
    dirty = rng.integers(1, 1 << 30, (n, V)).astype(np.int32)
    st = torch.from_numpy(dirty).to(DEV)
    prompt = (off - 20 + rng.integers(0, V + 40, 500)).astype(np.int64)
    pd = torch.from_numpy(prompt).to(DEV)
    _lib.check(lib.chatts_logit_state_reset(st[2].data_ptr(), V, off, pd.data_ptr(), len(prompt), _st()))
    torch.cuda.synchronize()
    got = st.cpu().numpy()
    assert np.array_equal(got[[0, 1, 3]], dirty[[0, 1, 3]])                       # no other row is touched
    assert np.array_equal(got[2], PROMPT_BIT * ref.prompt_mask(prompt, V, off).astype(np.int32))
    _lib.check(lib.chatts_logit_state_reset(st[1].data_ptr(), V, off, None, 0, _st()))       # no prompt: cleared only
    torch.cuda.synchronize()
    assert not st[1].any().item()
    # 40 updates of all four rows at once, with repeats and with tokens outside the slice
    st.zero_()
    _lib.check(lib.chatts_logit_state_reset(st[2].data_ptr(), V, off, pd.data_ptr(), len(prompt), _st()))
    toks = off - 3 + rng.integers(0, 60, (40, n)).astype(np.int64)                # a narrow range: many repeats; some ids below the slice
    toks[::7, 0] = off + V + 5                                                    # ... and some above
    td = torch.from_numpy(toks).to(DEV)
    for s in range(40):
        _lib.check(lib.chatts_logit_state_update(st.data_ptr(), V, n, V, off, td[s].data_ptr(), _st()))
    torch.cuda.synchronize()
    got = st.cpu().numpy()
    for b in range(n):
        want = ref.counts_of(toks[:, b], V, off)
        assert want.max() >= 2
        assert np.array_equal(got[b] & (PROMPT_BIT - 1), want), b
        assert np.array_equal((got[b] & PROMPT_BIT) != 0, ref.prompt_mask(prompt, V, off) if b == 2 else np.zeros(V, bool))


def test_two_runs_and_a_graph_replay_give_identical_bits(lib):
    V, off = 37984, 37984
    x, prompts, hists = _case(16, V, off)
    state = _state(prompts, hists, V, off)
    eager, _ = _apply(lib, x, state, ROWS16, off, runs=2)
    replay, after = _apply(lib, x, state, ROWS16, off, graph=True, runs=2)
    for o in (eager[1], replay[0], replay[1]):
        assert np.array_equal(o.view(np.uint32), eager[0].view(np.uint32))
    assert np.array_equal(after.view(np.uint32), x.view(np.uint32))
    # the same row gives the same bits in any row of the batch (no dependence on the row index)
    x2 = np.repeat(x[3:4], 3, axis=0)
    s2 = np.repeat(state[3:4], 3, axis=0)
    (g,), _ = _apply(lib, x2, s2, [ROWS16[10]] * 3, off)
    assert np.array_equal(g[0].view(np.uint32), g[1].view(np.uint32)) and np.array_equal(g[0].view(np.uint32), g[2].view(np.uint32))


def test_argument_errors(lib):
    x = torch.zeros((2, 64), device=DEV)
    st = torch.zeros((2, 64), dtype=torch.int32, device=DEV)
    out = torch.zeros((2, 64), device=DEV)
    ws = torch.zeros(int(lib.chatts_logit_controls_workspace(2)), dtype=torch.uint8, device=DEV)
    ok = dict(state=st.data_ptr(), state_stride=64, out=out.data_ptr(), out_stride=64)
    for bad in (dict(ok, state=None), dict(ok, out=None), dict(ok, out=x.data_ptr()), dict(ok, state_stride=63), dict(ok, out_stride=8)):
        a = _lib.LogitControlArgs(**bad)
        assert lib.chatts_logit_controls_apply(x.data_ptr(), 2, 64, 64, 0, C.byref(a), ws.data_ptr(), ws.numel(), _st()) == _lib.E_BADARG
    a = _lib.LogitControlArgs(**ok)
    assert lib.chatts_logit_controls_apply(x.data_ptr(), 2, 64, 64, 0, C.byref(a), ws.data_ptr(), 8, _st()) == _lib.E_WORKSPACE
    _lib.check(lib.chatts_logit_controls_apply(x.data_ptr(), 2, 64, 64, 0, C.byref(a), ws.data_ptr(), ws.numel(), _st()))   # all arrays NULL: a copy
    torch.cuda.synchronize()
    assert torch.equal(out, x)
