"""CPU: the inputs of tests/test_gpu_selection_edges.py are fair, and tests/selection_ref.py agrees with torch where torch has an answer.

check_draw grants its n_kept / kept_mass margins per ambiguous id (a probability within float32 rounding distance of a cut).  A row with
many such ids would let a wrong kept set through, so every (row, setting) the GPU test draws from must have at most 2 - a condition on the
inputs, checked here without a GPU."""
import numpy as np
import pytest
import torch

from tests import selection_ref as sel


@pytest.mark.parametrize("V,stride", sel.SAMPLER_SHAPES)
def test_sampled_rows_have_at_most_two_ids_near_a_cut(V, stride):
    rows = sel.sampled_rows(V)
    for kind, row in rows.items():
        assert not sel.is_degenerate(row), kind
    assert np.isfinite(rows["masked"][int(np.argmax(rows["plain"]))])          # the maximum survives the mask
    assert int(np.isfinite(rows["single"]).sum()) == 1
    if V == 4099:
        assert int(np.isfinite(rows["masked"]).sum()) == 384                    # top_k = 1000 reaches into the -inf entries
    worst = 0
    for kind, T, k, p in sel.sampler_settings(V):
        a = sel.ambiguous(rows[kind], T, k, p)
        worst = max(worst, a)
        assert a <= 2, (V, kind, T, k, p, a)
    print(f"V={V}: {len(sel.sampler_settings(V))} (row, setting) pairs, at most {worst} ambiguous ids")


@pytest.mark.parametrize("V,stride", sel.SHAPES)
def test_greedy_reference_is_torch_argmax_without_nan(V, stride):
    rows = sel.greedy_rows(V)
    for i, row in enumerate(rows):
        want = sel.greedy(row)
        if not np.isnan(row).any():
            assert want == int(torch.argmax(torch.from_numpy(row))), (V, i)
        elif np.isnan(row).all() or not (row[~np.isnan(row)] > -np.inf).any():
            assert want is None, (V, i)
        else:                                                                    # NaN skipped: torch.argmax of the row with NaN -> -inf
            assert want == int(torch.argmax(torch.nan_to_num(torch.from_numpy(row), nan=-np.inf, posinf=np.inf, neginf=-np.inf))), (V, i)
            assert not np.isnan(row[want])
    assert sel.greedy(rows[3]) == 0                                              # all -inf
    assert sel.greedy(rows[2]) == V - 1                                          # the only finite entry
    assert sel.greedy(rows[7]) is None                                           # all NaN
    assert [sel.is_degenerate(r) for r in rows[[0, 3, 4, 6, 7]]] == [False, True, True, True, True]


def test_greedy_reference_on_hand_made_rows():
    inf, nan = np.inf, np.nan
    assert sel.greedy([1.0, 3.0, 3.0, -inf]) == 1
    assert sel.greedy([-inf, -inf, -inf]) == 0
    assert sel.greedy([0.0, inf, 5.0, inf]) == 1
    assert sel.greedy([nan, 2.0, nan, 7.0, 7.0]) == 3
    assert sel.greedy([nan, -inf, -1.0]) == 2
    assert sel.greedy([nan, -inf, -inf]) is None and sel.greedy([nan, nan]) is None
    assert sel.greedy([nan, inf, 1.0]) == 1
    assert [sel.is_degenerate(r) for r in ([1.0, -inf], [-inf, -inf], [1.0, inf], [1.0, nan], [nan])] == [False, True, True, True, True]
