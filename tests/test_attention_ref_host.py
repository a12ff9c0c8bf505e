"""Host: the references, yardsticks and case lists of tests/attention_ref.py, which the GPU attention edge tests
(test_gpu_attention_edges.py) stand on.

For every case the GPU test runs (the sweep of the score offset included): the inputs really reach the profile's score range, the
truth is finite, the bar stays under the cap (a loose bar would hide a failure) and the float32 online softmax WITHOUT a fault passes
the float32-class bar (the bar is not too tight).  Per kernel family: each fault of `online32` is non-finite or more than 10 x above
the bar on at least one case (the bar is not blind).  Prototype figures: the faults gave 4e-2 .. 2.5, except newest_key_masked on
ramp_down (1.6e-7: the newest key carries almost no weight there) and on saw (8e-5) - which is why `newest` and `ramp_up` are in the
list."""
import math

import pytest
import torch

from tests import attention_ref as ar

FAMILIES = ("decode", "verify", "rows", "bf16x3", "mfma", "planes")
SPECS = ar.family_specs()
NOT_IN_THE_FAMILY = {"planes": {"combine_ignores_max"}}       # the planes kernel runs on one key split only: it has no combine


def test_ref64_is_the_suites_reference_and_row_err_is_per_row():
    g = torch.Generator().manual_seed(1)
    q, k, v = torch.randn((3, 4, 128), generator=g), torch.randn((2, 16, 128), generator=g), torch.randn((2, 16, 128), generator=g)
    want = ar.ref64(q, k, v, 5)
    # by hand: row 1 of head 3 (kv head 1) sees keys 0 .. 6
    s = (q[1, 3].double() @ k[1, :7].double().t()) / math.sqrt(128.0)
    assert torch.allclose(want[1, 3], torch.softmax(s, 0) @ v[1, :7].double(), rtol=1e-12, atol=0)
    got = want.clone()
    got[2, 1] *= 1.01                                    # one wrong row of 12: the per-row metric sees all of it
    assert abs(ar.row_err(got, want) - 0.01) < 1e-12


def test_split_yardstick_keeps_about_17_bits_and_drops_lo_lo():
    x = torch.randn(4096, generator=torch.Generator().manual_seed(2))
    hi, lo = ar._hi_lo(x)
    assert float(((hi + lo) - x.double()).abs().max() / x.abs().max()) < 2.0 ** -16
    assert torch.equal(hi.float().to(torch.bfloat16).double(), hi) and torch.equal(lo.float().to(torch.bfloat16).double(), lo)


def test_fused_inputs_round_trip():
    """raw -> norm + RoPE (host float64) gives the profile's targets back (without qk_norm: exactly the rotation's inverse)"""
    c = ar.make_case("shift+120", 69, 4, 2, 3, 40, 64, seed=9, fused=True)
    assert c["raw"].shape == (3, 8 * 128) and c["qn"] is None
    assert abs(c["smax"] - 120) < 60 and c["smin"] > 0
    assert torch.equal(c["k"][:, 40:43], c["knew64"].transpose(0, 1).float()) and torch.isnan(c["k"][:, 43:]).all()
    n = ar.make_case("shift+120", 69, 4, 2, 3, 40, 64, seed=9, fused=True, qk_norm=True)
    assert n["qn"] is not None and n["smax"] >= 60


@pytest.mark.parametrize("family", FAMILIES)
def test_every_case_reaches_its_scores_under_the_cap_and_the_faultless_form_passes(family):
    assert len(set(SPECS[family])) == len(SPECS[family])
    for spec, c, bar in ar.iter_cases(family):
        assert torch.isfinite(c["want"]).all(), spec
        assert max(abs(c["smax"]), abs(c["smin"])) >= 0.5 * c["target"], (spec, c["smax"], c["smin"])
        assert bar <= ar.BAR_CAP, (spec, c["y32"], c["y_split"])
        err = ar.row_err(ar.online32(c["q"], c["k"], c["v"], spec.pos0, ar.TILE[family], spec.splits), c["want"])
        f32_bar = ar.bar_of("rows", c["y32"], 0.0)
        assert err <= f32_bar, (spec, err, c["y32"], f32_bar)


@pytest.mark.parametrize("family", FAMILIES)
def test_every_fault_is_caught_on_some_case_of_the_family(family):
    missed = set(ar.FAULTS) - NOT_IN_THE_FAMILY.get(family, set())
    seen = {}
    for spec, c, bar in ar.iter_cases(family):
        if not missed:
            break
        if spec.max_ctx > 512:                         # (the long cases add nothing a short one does not show)
            continue
        for fault in sorted(missed):
            got = ar.online32(c["q"], c["k"], c["v"], spec.pos0, ar.TILE[family], spec.splits, fault)
            err = ar.row_err(got, c["want"])
            seen[fault] = max(seen.get(fault, 0.0), err if math.isfinite(err) else math.inf)
            if not torch.isfinite(got).all() or err > 10 * bar:
                missed.discard(fault)
    assert not missed, (missed, seen)
