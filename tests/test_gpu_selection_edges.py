"""GPU: token selection on masked, non-finite and padded logit rows, through the C-ABI, against the float64 rules of
tests/selection_ref.py (the contract at chatts_argmax / chatts_sample_batched in include/chatts_amd.h).

Every logits buffer here has its padding [vocab, stride) filled with NaN and every call a vocab_offset of 1000: a read of the padding, or a
use of the stride as the vocabulary, fails the test.  tests/test_selection_ref_host.py proves on the CPU that the sampled rows are fair
(at most 2 ids within float32 rounding distance of a cut)."""
import ctypes as C

import numpy as np
import pytest
import torch

from chatts_amd import _lib
from tests import logit_controls_ref as lcref
from tests import selection_ref as sel

pytestmark = pytest.mark.gpu
DEV = "cuda"
OFF = sel.VOCAB_OFFSET
CANARY = 12345.0
PROMPT_BIT = 1 << 30


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _padded(rows, stride):
    """float32 rows [B, V] -> device [B, stride] with NaN in the padding"""
    rows = np.asarray(rows, dtype=np.float32)
    buf = np.full((rows.shape[0], stride), np.nan, dtype=np.float32)
    buf[:, :rows.shape[1]] = rows
    return torch.from_numpy(buf).to(DEV)


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _lp_close(got, want):
    """tests/test_gpu_logprobs.py's tolerance"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.isfinite(want).all() and np.isfinite(got).all()
    assert np.all(np.abs(got - want) <= 1e-5 + 1e-7 * np.abs(want)), np.abs(got - want).max()


class _Out:
    """the output cells of one selection launch, pre-filled so that an unwritten cell shows"""

    def __init__(self, b, steps, pos, out_stride):
        self.tok = torch.full((b,), -1, dtype=torch.int64, device=DEV)
        self.tl = torch.full((b,), CANARY, dtype=torch.float32, device=DEV)
        self.nk = torch.full((b,), -7, dtype=torch.int32, device=DEV)
        self.km = torch.full((b,), CANARY, dtype=torch.float32, device=DEV)
        self.step = torch.tensor(steps, dtype=torch.int32, device=DEV)
        self.pos = torch.tensor(pos, dtype=torch.int32, device=DEV)
        self.out = torch.full((b, out_stride), -1, dtype=torch.int64, device=DEV)

    def host(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in ("tok", "tl", "nk", "km", "step", "pos", "out")}


def _sample(lib, logits, vocab, steps, pos, pos_limit, out_stride, scalar=None, rows=None):
    """chatts_sample_batched on a padded device buffer; scalar = (T, top_k, top_p, seed) or rows = [(T, top_k, top_p, seed)] per row"""
    b, stride = logits.shape
    o = _Out(b, steps, pos, out_stride)
    if rows is not None:
        par = [torch.tensor([r[0] for r in rows], dtype=torch.float32, device=DEV), torch.tensor([r[1] for r in rows], dtype=torch.int32, device=DEV),
               torch.tensor([r[2] for r in rows], dtype=torch.float32, device=DEV), torch.tensor([r[3] for r in rows], dtype=torch.int32, device=DEV)]
        sa = _lib.SamplingArgs(temperature=0.0, top_k=0, top_p=0.0, seed=0, n_kept=o.nk.data_ptr(), kept_mass=o.km.data_ptr(),
                               temperature_rows=par[0].data_ptr(), top_k_rows=par[1].data_ptr(), top_p_rows=par[2].data_ptr(),
                               seed_rows=par[3].data_ptr())
    else:
        sa = _lib.SamplingArgs(temperature=scalar[0], top_k=scalar[1], top_p=scalar[2], seed=scalar[3], n_kept=o.nk.data_ptr(),
                               kept_mass=o.km.data_ptr())
    _lib.check(lib.chatts_sample_batched(logits.data_ptr(), b, stride, vocab, OFF, C.byref(sa), o.tok.data_ptr(), o.tl.data_ptr(),
                                         o.out.data_ptr(), out_stride, o.step.data_ptr(), o.pos.data_ptr(), pos_limit, _st()))
    return o.host()


# ---- greedy ---------------------------------------------------------------------------------------------------------------------------
G_STEPS = [0, 1, 2, 3, 0, 1, 2, 5]           # row 7: the counter is past out_tokens' 4 cells - nothing appended, the counter still moves
G_POS = [5, -1, 9, 10, 3, 0, -1, 10]         # parked (-1) stays parked; 10 = pos_limit saturates
G_POS_AFTER = [6, -1, 10, 10, 4, 1, -1, 10]
G_LIMIT, G_OUT = 10, 4


def _greedy_forms(lib, logits, vocab):
    """the batch through every greedy form -> {form: host outputs}"""
    b, stride = logits.shape
    ws = torch.empty(int(lib.chatts_argmax_workspace(b)), dtype=torch.uint8, device=DEV)
    forms = {}
    for name, use_ws in (("one launch", False), ("two launches", True)):
        o = _Out(b, G_STEPS, G_POS, G_OUT)
        _lib.check(lib.chatts_argmax_batched_ws(logits.data_ptr(), b, stride, vocab, OFF, o.tok.data_ptr(), o.tl.data_ptr(), o.out.data_ptr(),
                                                G_OUT, o.step.data_ptr(), o.pos.data_ptr(), G_LIMIT, ws.data_ptr() if use_ws else None,
                                                ws.numel() if use_ws else 0, _st()))
        forms[name] = o.host()
    forms["sampler, temperature 0"] = _sample(lib, logits, vocab, G_STEPS, G_POS, G_LIMIT, G_OUT, rows=[(0.0, 20, 0.9, 3)] * b)
    return forms


@pytest.mark.parametrize("vocab,stride", sel.SHAPES)
def test_greedy_forms_on_masked_non_finite_and_padded_rows(lib, vocab, stride):
    """Rules 1-4: the one-workgroup argmax, the two-launch argmax (vocab >= 4096) and the temperature-0 rows of the per-row sampler return
    selection_ref.greedy's token on a plain row, a 90 % -inf row, a row whose only finite entry is the last, an all -inf row, a row with
    two +inf, a row of float32 extremes / denormals / a tie, a row with 5 % NaN; on the all-NaN row (and wherever the reference leaves the
    token free) a token of the row, the same in every form and run.  token_logit is logits[token] bit for bit; step, pos and out_tokens
    move for every row."""
    rows = sel.greedy_rows(vocab)
    logits = _padded(rows, stride)
    want = [sel.greedy(r) for r in rows]
    assert want[3] == 0 and want[7] is None
    runs = [_greedy_forms(lib, logits, vocab), _greedy_forms(lib, logits, vocab)]
    first = runs[0]["one launch"]
    print(f"V={vocab}/{stride}: reference {want}, device {(first['tok'] - OFF).tolist()}")
    for run in runs:
        for name, got in run.items():
            tok = got["tok"] - OFF
            for i in range(8):
                assert 0 <= tok[i] < vocab, (name, i, int(got["tok"][i]))
                if want[i] is not None:
                    assert tok[i] == want[i], (name, i, int(tok[i]), want[i])
                assert _bits(got["tl"][i]) == _bits(rows[i, tok[i]]), (name, i)
                cell = G_STEPS[i]
                assert got["out"][i].tolist() == [int(got["tok"][i]) if c == cell else -1 for c in range(G_OUT)], (name, i)
            assert got["step"].tolist() == [s + 1 for s in G_STEPS], name
            assert got["pos"].tolist() == G_POS_AFTER, name
            assert np.array_equal(got["tok"], first["tok"]), name               # every form, both runs: the same tokens
            if name.startswith("sampler"):
                assert got["nk"].tolist() == [1] * 8 and got["km"].tolist() == [0.0] * 8
    # row 0 alone through the single-sequence entry point
    tok = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    val = torch.full((1,), CANARY, device=DEV)
    outt = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    step = torch.tensor([2], dtype=torch.int32, device=DEV)
    pos = torch.tensor([10], dtype=torch.int32, device=DEV)
    _lib.check(lib.chatts_argmax(logits.data_ptr(), vocab, OFF, tok.data_ptr(), val.data_ptr(), outt.data_ptr(), step.data_ptr(), pos.data_ptr(),
                                 _st()))
    torch.cuda.synchronize()
    assert tok.item() == want[0] + OFF and _bits(val.cpu().numpy())[0] == _bits(rows[0, want[0]])
    assert outt.tolist() == [-1, -1, want[0] + OFF, -1] and step.item() == 3 and pos.item() == 11


def test_greedy_all_nan_row_alone(lib):
    """chatts_argmax on an all-NaN and on an all -inf row: a token of the row (0 for -inf), its bits, and the side effects"""
    V = 1003
    for fill in (np.nan, -np.inf):
        logits = _padded(np.full((1, V), fill, dtype=np.float32), V + 1)
        tok = torch.full((1,), -1, dtype=torch.int64, device=DEV)
        val = torch.full((1,), CANARY, device=DEV)
        outt = torch.full((4,), -1, dtype=torch.int64, device=DEV)
        step = torch.tensor([1], dtype=torch.int32, device=DEV)
        pos = torch.tensor([7], dtype=torch.int32, device=DEV)
        _lib.check(lib.chatts_argmax(logits.data_ptr(), V, OFF, tok.data_ptr(), val.data_ptr(), outt.data_ptr(), step.data_ptr(),
                                     pos.data_ptr(), _st()))
        torch.cuda.synchronize()
        assert OFF <= tok.item() < OFF + V
        if fill == -np.inf:
            assert tok.item() == OFF
        assert _bits(val.cpu().numpy())[0] == _bits(np.float32(fill))
        assert outt.tolist() == [-1, tok.item(), -1, -1] and step.item() == 2 and pos.item() == 8


# ---- sampler, regular rows -------------------------------------------------------------------------------------------------------------
_ROWS = {}


def _sampled_rows(V):
    if V not in _ROWS:
        _ROWS[V] = sel.sampled_rows(V)
    return _ROWS[V]


def _settings():
    return [pytest.param(V, stride, kind, T, k, p, id=f"{V}-{kind}-T{T:g}-k{k}-p{p:g}")
            for V, stride in sel.SAMPLER_SHAPES for kind, T, k, p in sel.sampler_settings(V)]


@pytest.mark.parametrize("V,stride,kind,T,k,p", _settings())
def test_sampler_regular_rows_with_masked_ids_and_padding(lib, V, stride, kind, T, k, p):
    """Rule 5, scalar and per-row mode: every draw is valid under oracle/sampler.py's float64 rule (check_draw, margins unchanged) on a
    plain row, a 90 % -inf row and a row with one finite entry; a -inf id is never drawn and never counted."""
    row = _sampled_rows(V)[kind]
    ctx = sel.DrawContext(row, T, k, p)
    assert ctx.ambiguous <= 2
    steps = sel.SAMPLER_STEPS + [sel.SAMPLER_STEPS[0]]                        # row 4 repeats row 0's draw counter
    b = len(steps)
    logits = _padded(np.tile(row, (b, 1)), stride)
    seed = 99
    for mode in ("scalar", "per-row"):
        if mode == "scalar":
            got = _sample(lib, logits, V, steps, [4] * b, 0, 8, scalar=(T, k, p, seed))
        else:
            got = _sample(lib, logits, V, steps, [4] * b, 0, 8, rows=[(T, k, p, seed)] * b)
        assert got["step"].tolist() == [s + 1 for s in steps] and got["pos"].tolist() == [5] * b
        for i in range(b):
            t = int(got["tok"][i]) - OFF
            assert 0 <= t < V, (mode, i, int(got["tok"][i]))
            assert row[t] != -np.inf, (mode, i, t)
            assert _bits(got["tl"][i]) == _bits(row[t])
            assert got["out"][i].tolist() == [int(got["tok"][i]) if c == steps[i] else -1 for c in range(8)]
            sel.check_draw(row, got["tok"][i], T, k, p, seed, i if mode == "scalar" else 0, steps[i], got["nk"][i], got["km"][i],
                           vocab_offset=OFF, ctx=ctx)
            assert got["nk"][i] <= int(np.isfinite(row).sum())
        if mode == "per-row":
            assert got["tok"][4] == got["tok"][0]                             # same settings, seed and step in another row: the same token
        if T == 1e-3:
            assert (got["nk"] == int((row == row.max()).sum())).all()         # everything but the maxima is below the 2^-40 floor
        if kind == "single":
            assert (got["tok"] - OFF == (2 * V) // 3).all() and (got["nk"] == 1).all()


@pytest.mark.parametrize("V,stride", sel.SAMPLER_SHAPES)
def test_sampler_single_finite_entry_is_drawn_at_every_counter(lib, V, stride):
    """one finite entry among -inf: whatever the variate (64 draw counters, both modes), that id is drawn"""
    row = _sampled_rows(V)["single"]
    steps = list(range(64))
    logits = _padded(np.tile(row, (64, 1)), stride)
    for got in (_sample(lib, logits, V, steps, [0] * 64, 0, 64, scalar=(1.0, 0, 1.0, 7)),
                _sample(lib, logits, V, steps, [0] * 64, 0, 64, rows=[(0.8, 40, 0.95, 7)] * 64)):
        assert (got["tok"] - OFF == (2 * V) // 3).all()
        assert (got["nk"] == 1).all() and np.allclose(got["km"], 1.0, atol=1e-6)
        assert got["step"].tolist() == [s + 1 for s in steps] and got["pos"].tolist() == [1] * 64


# ---- sampler, degenerate rows ----------------------------------------------------------------------------------------------------------
D_SETTINGS = [(0.7, 20, 0.9, 1234), (1.0, 0, 1.0, 77), (0.5, 0, 0.95, 5), (1.0, 50, 1.0, 9), (0.2, 0, 0.5, 11), (1.0, 0, 1.0, 42)]
D_STEPS = [3, 0, 7, 2, 1, 6]
D_POS = [4, 9, -1, 10, 0, 4]                 # row 2 is parked, row 3 sits on pos_limit 10
D_POS_AFTER = [5, 10, -1, 10, 1, 5]


def _degenerate_rows(V):
    base, _ = sel.base_row(V)
    rows = np.tile(base, (6, 1))
    rows[1, :] = -np.inf
    rows[2, V // 2] = np.inf
    rows[3, [1 % V, V // 3, V - 1]] = np.nan
    rows[4, :] = np.nan
    rows[5] = base[::-1]
    return rows


@pytest.mark.parametrize("V,stride", [(17, 20), (1003, 1003), (4099, 4100)])
def test_sampler_degenerate_rows_select_greedily_and_leave_the_others_alone(lib, V, stride):
    """Rules 6 and 7: an all -inf row, a row with a +inf, a row with three NaN and an all-NaN row between two regular rows, one launch.
    The degenerate rows return the greedy reference's token with token_logit = logits[token], n_kept = 1, kept_mass = 0, and move step, pos
    and out_tokens; the regular rows draw bit for bit what they draw alone; a second launch gives identical outputs."""
    rows = _degenerate_rows(V)
    assert [sel.is_degenerate(r) for r in rows] == [False, True, True, True, True, False]
    logits = _padded(rows, stride)
    want = [sel.greedy(r) for r in rows]
    assert want[1] == 0 and want[2] == V // 2 and want[3] is not None and want[4] is None
    got = _sample(lib, logits, V, D_STEPS, D_POS, 10, 8, rows=D_SETTINGS)
    again = _sample(lib, logits, V, D_STEPS, D_POS, 10, 8, rows=D_SETTINGS)
    print(f"V={V}: tokens {(got['tok'] - OFF).tolist()} n_kept {got['nk'].tolist()} kept_mass {got['km'].tolist()} step {got['step'].tolist()}")
    for key in got:
        assert got[key].tobytes() == again[key].tobytes(), key
    assert got["step"].tolist() == [s + 1 for s in D_STEPS] and got["pos"].tolist() == D_POS_AFTER
    for i in range(6):
        t = int(got["tok"][i]) - OFF
        assert 0 <= t < V, (i, int(got["tok"][i]))
        assert _bits(got["tl"][i]) == _bits(rows[i, t]), i
        assert got["out"][i].tolist() == [int(got["tok"][i]) if c == D_STEPS[i] else -1 for c in range(8)], i
    for i in (1, 2, 3, 4):
        if want[i] is not None:
            assert int(got["tok"][i]) - OFF == want[i], (i, int(got["tok"][i]) - OFF, want[i])
        assert got["nk"][i] == 1 and got["km"][i] == 0.0, i
    for i in (0, 5):                                                          # in per-row mode a row depends on its seed and step only
        T, k, p, seed = D_SETTINGS[i]
        assert sel.ambiguous(rows[i], T, k, p) <= 2
        sel.check_draw(rows[i], got["tok"][i], T, k, p, seed, 0, D_STEPS[i], got["nk"][i], got["km"][i], vocab_offset=OFF)
        alone = _sample(lib, logits[i:i + 1], V, [D_STEPS[i]], [D_POS[i]], 10, 8, rows=[D_SETTINGS[i]])
        for key in ("tok", "tl", "nk", "km", "step", "pos", "out"):
            assert alone[key][0].tobytes() == got[key][i].tobytes(), (i, key)
    # scalar mode: the same degenerate rows; the regular rows draw what they draw next to four regular neighbours (the row index salts
    # the variate, so "alone" is not the comparison here)
    T, k, p, seed = D_SETTINGS[0]
    sc = _sample(lib, logits, V, D_STEPS, D_POS, 10, 8, scalar=(T, k, p, seed))
    calm = rows.copy()
    calm[1:5] = rows[0]
    ref = _sample(lib, _padded(calm, stride), V, D_STEPS, D_POS, 10, 8, scalar=(T, k, p, seed))
    assert sc["step"].tolist() == [s + 1 for s in D_STEPS] and sc["pos"].tolist() == D_POS_AFTER
    for i in (1, 2, 3, 4):
        t = int(sc["tok"][i]) - OFF
        assert 0 <= t < V and (want[i] is None or t == want[i]), (i, t, want[i])
        assert t == int(got["tok"][i]) - OFF                                  # the per-row launch's token: one greedy rule
        assert _bits(sc["tl"][i]) == _bits(rows[i, t]) and sc["nk"][i] == 1 and sc["km"][i] == 0.0
        assert sc["out"][i].tolist() == [int(sc["tok"][i]) if c == D_STEPS[i] else -1 for c in range(8)]
    for i in (0, 5):
        assert sel.ambiguous(rows[i], T, k, p) <= 2
        sel.check_draw(rows[i], sc["tok"][i], T, k, p, seed, i, D_STEPS[i], sc["nk"][i], sc["km"][i], vocab_offset=OFF)
        for key in ("tok", "tl", "nk", "km", "step", "pos", "out"):
            assert sc[key][i].tobytes() == ref[key][i].tobytes(), (i, key)


# ---- the chain min_p -> sampler --------------------------------------------------------------------------------------------------------
C_ROWS = [(1.3, 0.5, 0.5, 0.8), (1.0, 0.0, 0.0, 1.0), (2.0, -1.0, 0.25, 0.6)]      # (repetition, frequency, presence, temperature) per row
C_SAMPLING = [(0, 1.0, 21), (40, 0.95, 22), (0, 0.9, 23)]                           # (top_k, top_p, seed) per row


@pytest.mark.parametrize("min_p", [0.05, 0.5, 1.0])
@pytest.mark.parametrize("V,stride", [(4099, 4100), (19009, 19012)])
def test_min_p_output_feeds_the_sampler(lib, V, stride, min_p):
    """chatts_logit_controls_apply (penalties on a third of the ids, min_p) writes -inf below its cut; chatts_sample_batched draws from
    that buffer.  The token is alive in the float64 reference (up to the penalty bound at the cut), valid under check_draw on the device's
    own row, and with min_p = 1 one of the maxima."""
    rng = np.random.default_rng([V, int(min_p * 100)])
    x = (rng.standard_normal((3, V)) * 3.0).astype(np.float32)
    cnt = np.zeros((3, V), dtype=np.int64)
    inp = np.zeros((3, V), dtype=bool)
    for b in range(3):
        third = np.arange(b, V, 3)
        cnt[b, third] = rng.integers(0, 4, third.size)                          # 0 = seen in the prompt only
        inp[b, third] = True
    st = np.zeros((3, stride), dtype=np.int32)                                  # the state rows are padded like the logits
    st[:, :V] = cnt + PROMPT_BIT * inp
    state = torch.from_numpy(st).to(DEV)
    lg = _padded(x, stride)
    out = torch.full((3, stride), float("nan"), device=DEV)
    par = [torch.tensor([r[i] for r in C_ROWS], dtype=torch.float32, device=DEV) for i in range(4)]
    mp = torch.full((3,), min_p, dtype=torch.float32, device=DEV)
    ws = torch.zeros(int(lib.chatts_logit_controls_workspace(3)), dtype=torch.uint8, device=DEV)
    args = _lib.LogitControlArgs(state=state.data_ptr(), state_stride=stride, out=out.data_ptr(), out_stride=stride, repetition_rows=par[0].data_ptr(),
                                 frequency_rows=par[1].data_ptr(), presence_rows=par[2].data_ptr(), min_p_rows=mp.data_ptr(),
                                 temperature_rows=par[3].data_ptr())
    _lib.check(lib.chatts_logit_controls_apply(lg.data_ptr(), 3, stride, V, OFF, C.byref(args), ws.data_ptr(), ws.numel(), _st()))
    steps = [0, 5, 123]
    rows = [(C_ROWS[b][3], *C_SAMPLING[b]) for b in range(3)]
    got = _sample(lib, out, V, steps, [4, 4, 4], 0, 128, rows=rows)
    dev = out.cpu().numpy()
    assert np.isnan(dev[:, V:]).all()                                           # the controls left the padding alone
    assert got["step"].tolist() == [1, 6, 124] and got["pos"].tolist() == [5, 5, 5]
    for b in range(3):
        r, f, p, T = C_ROWS[b]
        row = dev[b, :V]
        assert not sel.is_degenerate(row)
        t = int(got["tok"][b]) - OFF
        assert 0 <= t < V and row[t] != -np.inf and _bits(got["tl"][b]) == _bits(row[t])
        pen, cut = lcref.apply(x[b], inp[b], cnt[b], r, f, p, min_p, T)
        raw = lcref.penalise(x[b], inp[b], cnt[b], r, f, p)
        bound = lcref.penalty_bound(x[b], cnt[b], r, f, p)
        band = bound[t] + bound[int(np.argmax(raw))] + 4 * lcref.EPS * abs(T * np.log(min_p))
        assert raw[t] >= cut - band, (b, t, raw[t], cut, band)                  # alive in the reference, up to its bound at the cut
        top_k, top_p, seed = C_SAMPLING[b]
        print(f"V={V} min_p={min_p} row {b}: {int((row != -np.inf).sum())} survivors ({int((pen != -np.inf).sum())} in the reference), "
              f"token {t}, n_kept {got['nk'][b]}")
        sel.check_draw(row, got["tok"][b], T, top_k, top_p, seed, 0, steps[b], got["nk"][b], got["km"][b], vocab_offset=OFF)
        if min_p == 1.0:
            assert row[t] == row.max() and got["nk"][b] == int((row == row.max()).sum())


# ---- logprobs with NaN logits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [4099, 19008])
def test_logprobs_ignore_nan_logits(lib, V):
    """csrc/logprobs.hip: "NaN logits are never selected or counted".  A row with NaN at 5 % of the ids (the last id among them, and the
    id of the largest logit): logprob, rank and the top-5 equal the float64 log_softmax over the non-NaN entries, within
    tests/test_gpu_logprobs.py's tolerance; no NaN id is listed."""
    k, batch, out_stride = 5, 3, 2
    rng = np.random.default_rng(V)
    x = (rng.standard_normal((batch, V)) * 3.0).astype(np.float32)
    tokens = []
    for b in range(batch):
        nan = rng.random(V) < 0.05
        nan[[0, V - 1, int(np.argmax(x[b]))]] = True
        x[b, nan] = np.nan
        ok = np.flatnonzero(~nan)
        tokens.append(int(ok[len(ok) // 2]) if b else int(ok[np.argmax(x[b, ok])]))      # row 0: the best non-NaN id, rank 1
    stride = V + 4
    lg = _padded(x, stride)
    tok = torch.tensor([t + OFF for t in tokens], dtype=torch.int64, device=DEV)
    step = torch.tensor([1, 2, 1], dtype=torch.int32, device=DEV)
    lp = torch.full((batch, out_stride), float("nan"), device=DEV)
    rank = torch.full((batch, out_stride), -1, dtype=torch.int32, device=DEV)
    tid = torch.full((batch, out_stride, k), -1, dtype=torch.int32, device=DEV)
    tlp = torch.full((batch, out_stride, k), float("nan"), device=DEV)
    ws = torch.zeros(int(lib.chatts_logprobs_workspace(batch, k)), dtype=torch.uint8, device=DEV)
    _lib.check(lib.chatts_logprobs_batched(lg.data_ptr(), batch, stride, V, OFF, k, tok.data_ptr(), step.data_ptr(), out_stride, lp.data_ptr(),
                                           rank.data_ptr(), tid.data_ptr(), tlp.data_ptr(), ws.data_ptr(), ws.numel(), _st()))
    torch.cuda.synchronize()
    lp, rank, tid, tlp = lp.cpu().numpy(), rank.cpu().numpy(), tid.cpu().numpy(), tlp.cpu().numpy()
    for b in range(batch):
        cell = int(step[b]) - 1
        l = x[b].astype(np.float64)
        ok = ~np.isnan(l)
        m = l[ok].max()
        lse = m + np.log(np.exp(l[ok] - m).sum())
        t = tokens[b]
        _lp_close([lp[b, cell]], [l[t] - lse])
        assert rank[b, cell] == 1 + int((l[ok] > l[t]).sum()) + int((l[:t][ok[:t]] == l[t]).sum())
        if b == 0:
            assert rank[b, cell] == 1
        ids = np.flatnonzero(ok)
        order = ids[np.lexsort((ids, -l[ids]))][:k]
        assert (tid[b, cell] - OFF).tolist() == order.tolist()
        assert ok[tid[b, cell] - OFF].all()
        _lp_close(tlp[b, cell], l[order] - lse)
