"""tests/linear_ref.py on the CPU: the bars of test_gpu_linear_edges.py are neither blind nor too tight.

Every case of every list passes its own bar under the fault-free float32 emulation of its kernel family and stays under BAR_CAP; the
profiles are what they claim to be; each planted fault lands at least 10 x above the bar on some case of each family it applies to; and
the gap in the suite's older check is written down: two of the faults pass `rel_err < 2e-5`, the norm-wise bar of test_gpu_kernels.py."""
import pytest
import torch

from tests import linear_ref as lr
from tests.util import rel_err

OLD_BAR = 2e-5


@pytest.mark.parametrize("family", list(lr.LISTS))
def test_the_fault_free_emulation_passes_every_bar(family):
    specs = lr.LISTS[family]
    assert specs
    for s in specs:
        c = lr.build(s)
        assert torch.isfinite(c["emu"]).all() and torch.isfinite(c["want"]).all() and (c["S"] >= 0).all(), s
        assert lr.MARGIN * c["y"] <= lr.BAR_CAP, (s, c["y"])
        use, at = lr.bar_use(c["emu"], c["want"], c["bar"])
        assert use <= 1.0, (s, use, at)
        if s.post:
            use, at = lr.bar_use(lr.post32(s, c, c["emu"]), c["want_post"], c["bar_post"])
            assert use <= 1.0, (s, "post", use, at)


def test_case_lists_cover_what_they_claim():
    per = {f: {s.profile for s in specs} for f, specs in lr.LISTS.items()}
    for f, profiles in per.items():
        assert {"gauss", "outlier", "cancel", "zero_rows"} <= profiles, f
    assert "resid_stream" in per["gemv"] & per["bf16x2"] & per["stream"] & per["ring"] & per["epi"]
    assert any(s.profile == "wide_norm" and s.norm for s in lr.GEMV) and any(s.profile == "wide_norm" and s.post for s in lr.EPILOGUES)
    assert {s.fmt for s in lr.GEMV} == {"bf16", "fp8", "int8", "int4g16", "int4g128"}
    assert {(s.kernel, s.sk) for s in lr.GEMV if s.fmt == "bf16"} == {("gemv_ldsx", 1), ("gemv_ksplit", 2), ("gemv_ksplit", 3)}
    assert {len(lr.split_ranges(s)) for s in lr.RING} == {1, 3} and {len(lr.split_ranges(s)) for s in lr.STREAM} == {1, 2, 3}
    uneven = [s for s in lr.all_specs() if s.family != "gemv" and len({k1 - k0 for k0, k1 in lr.split_ranges(s)}) > 1]
    assert {s.family for s in uneven} == {"bf16x2", "stream", "ring", "epi"}        # a shorter last split on every split-K path
    assert len(lr.all_specs()) == len(set(lr.all_specs()))


def test_resid_stream_hides_the_product():
    specs = [s for s in lr.all_specs() if s.profile == "resid_stream"]
    assert specs
    for s in specs:
        c = lr.build(s)
        product = (c["want"] - c["resid"].double()).abs()
        assert float((c["resid"].double().abs() / product).median()) >= 100, s


def test_cancel_cases_cancel():
    specs = [s for s in lr.all_specs() if s.profile == "cancel"]
    assert specs
    for s in specs:
        c = lr.build(s)
        assert float((c["want"].abs() / c["S"]).median()) <= 1e-3, s


def test_zero_rows_are_bias_plus_resid():
    for s in (s for s in lr.all_specs() if s.profile == "zero_rows" and s.epi == lr.EPI_RESID):
        c = lr.build(s)
        for row in (0, s.m - 1):
            assert torch.equal(c["want"][row], c["bias"].double() + c["resid"][row].double()), s
            assert torch.equal(c["emu"][row], c["bias"] + c["resid"][row]), s          # one float32 addition


def _worst_use(fault, family, enough=10.0):
    """the largest |emulation with the fault - want| / bar over the family's cases (it stops at the first case that reaches `enough`), and
    how many cases the fault applied to"""
    worst, applies = 0.0, 0
    for s in lr.all_specs():
        if s.family != family:
            continue
        c = lr.build(s)
        out = lr.emulate(s, c, fault)
        if out is None:
            continue
        applies += 1
        worst = max(worst, lr.bar_use(out, c["want"], c["bar"])[0])
        if worst >= enough:
            break
    return worst, applies


@pytest.mark.parametrize("fault", lr.FAULTS)
def test_every_fault_lands_ten_times_above_the_bar(fault):
    for family in lr.fault_families(fault):
        worst, applies = _worst_use(fault, family)
        assert applies > 0 and worst >= 10.0, (fault, family, worst, applies)


def test_the_norm_wise_bar_lets_a_dropped_lo_plane_through_under_a_residual():
    """the gap: a kernel that drops the lo plane everywhere (plain bf16 activations) passes rel_err < 2e-5 on every resid_stream case of
    the plane kernels - and is caught by the componentwise bar on each of them"""
    specs = [s for s in lr.all_specs() if s.profile == "resid_stream" and s.family in lr.SPLIT_FAMILIES]
    assert specs
    for s in specs:
        c = lr.build(s)
        out = lr.emulate(s, c, "lo_plane_dropped")
        assert rel_err(out.numpy(), c["want"].numpy()) < OLD_BAR, s
        assert lr.bar_use(out, c["want"], c["bar"])[0] > 1.0, s
    assert max(lr.bar_use(lr.emulate(s, lr.build(s), "lo_plane_dropped"), lr.build(s)["want"], lr.build(s)["bar"])[0] for s in specs) >= 10.0


def test_the_norm_wise_bar_lets_a_wrong_corner_bias_through_at_the_largest_n():
    """the gap: one corner element with its neighbour's bias at the widest output of the lists passes rel_err < 2e-5"""
    n_max = max(s.n for s in lr.all_specs() if s.family != "epi")
    specs = [s for s in lr.all_specs() if s.n == n_max and s.profile == "resid_stream" and s.family == "ring"]
    assert specs and n_max == 416
    s = max(specs, key=lambda s: s.m * s.k)
    c = lr.build(s)
    out = lr.emulate(s, c, "corner_takes_neighbour_bias")
    assert rel_err(out.numpy(), c["want"].numpy()) < OLD_BAR
    assert lr.bar_use(out, c["want"], c["bar"])[0] >= 10.0


@pytest.mark.parametrize("profile,t,hidden,seed", lr.RMSNORM)
def test_rmsnorm_cases(profile, t, hidden, seed):
    c = lr.rms_case(profile, t, hidden, seed)
    assert torch.isfinite(c["want"]).all() and lr.MARGIN * c["y"] <= lr.BAR_CAP
    if profile == "zero_rows":
        assert bool((c["want"][0] == 0).all()) and bool((c["want"][t - 1] == 0).all())
