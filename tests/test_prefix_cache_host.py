"""The prefix-reuse policy (chatts_amd/prefix_cache.py) on the CPU: common-prefix length, which slot's resident prefix a request
matches (ties, exclusions), which free slot it takes, and when two <ts> placeholder tokens count as the same token."""
import numpy as np
import torch

from chatts_amd import prefix_cache as pc

TS0 = 1000          # the <ts> placeholder id of these prompts (text ids stay below it)


def _series(values, lmax):
    """[n, 2 * lmax, 1] (value, mask) pairs, zero-padded - the layout ChatTSProcessor emits"""
    out = np.zeros((len(values), lmax, 2), dtype=np.float32)
    for i, v in enumerate(values):
        out[i, :len(v), 0] = v
        out[i, :len(v), 1] = 1.0
    return torch.from_numpy(out.reshape(len(values), 2 * lmax, 1))


def test_common_prefix_len():
    assert pc.common_prefix_len([], [1, 2]) == 0
    assert pc.common_prefix_len([1, 2, 3], [1, 2, 3]) == 3
    assert pc.common_prefix_len([1, 2, 3], [1, 2]) == 2
    assert pc.common_prefix_len([1, 2], [1, 2, 3]) == 2
    assert pc.common_prefix_len([1, 2, 3], [1, 5, 3]) == 1
    assert pc.common_prefix_len([(b"d", 0), 7], [(b"d", 0), 7]) == 2
    assert pc.common_prefix_len([(b"d", 0), 7], [(b"d", 1), 7]) == 0


def test_match_prefix_takes_the_longest_prefers_the_slot_itself_on_a_tie_and_skips_excluded_slots():
    req = list(range(40))
    slots = [req[:20], req[:30], req[:30] + [99], [], [5] + req]
    assert pc.match_prefix(slots, req, 0) == (30, 1)                    # longest; the first of equals
    assert pc.match_prefix(slots, req, 2) == (30, 2)                    # a tie goes to the slot itself (zero copy)
    assert pc.match_prefix(slots, req, 0, exclude=(1,)) == (30, 2)
    assert pc.match_prefix(slots, req, 2, exclude=(2,)) == (30, 1)
    assert pc.match_prefix(slots, req, -1, exclude=(1, 2)) == (20, 0)
    assert pc.match_prefix(slots, req[:10], 0) == (10, 0)               # the request itself bounds the match
    # nothing in common: no source, not even the slot itself (the tie rule needs a match longer than 0)
    assert pc.match_prefix([[7], [], [5] + req], req, 1) == (0, -1)
    assert pc.match_prefix([[], []], req, 0) == (0, -1)


def test_pick_slot_takes_the_best_match_only_at_the_threshold_else_the_least_resident_slot():
    M = pc.MIN_REUSE
    assert M == 16
    req = list(range(100))
    slots = [list(range(500, 550)), req[:M], req[:M - 1], [1], req[:M + 10]]
    assert pc.pick_slot(slots, [0, 1, 2, 3, 4], req) == 4               # the best match
    assert pc.pick_slot(slots, [0, 1, 2, 3], req) == 1                  # a match of exactly the threshold is taken
    assert pc.pick_slot(slots, [0, 2, 3], req) == 3                     # M - 1 in common: the fewest resident tokens instead
    assert pc.pick_slot(slots, [0, 2], req) == 2
    assert pc.pick_slot([[], [], [3]], [2, 1, 0], req) == 1             # equally empty: the first in free_slots order
    assert pc.pick_slot(slots, [1, 3], [9] * 20) == 3                   # no match at all


def test_token_idents_text_tokens_are_their_ids_and_placeholders_digest_series_and_patch_index():
    a = np.arange(40, dtype=np.float32)
    b = a.copy()
    b[37] += 1.0                                                        # differs in the last patch only
    full = [1, 2, TS0, TS0, TS0, 3, TS0, TS0, TS0, 4]
    counts = [3, 3]
    lengths = [40, 40]
    same = pc.token_idents(full, _series([a, a], 48), lengths, counts, TS0)
    assert [same[i] for i in (0, 1, 5, 9)] == [1, 2, 3, 4]
    assert [p for _, p in (same[i] for i in (2, 3, 4))] == [0, 1, 2]
    assert same[2:5] == same[6:9]                                       # equal (value, mask) rows and patch indices
    assert same[2] != same[3]                                           # same series, other patch
    diff = pc.token_idents(full, _series([a, b], 48), lengths, counts, TS0)
    assert diff[:6] == same[:6]
    assert diff[2:5] != diff[6:9] and diff[6] != same[6]                # one value differs: every placeholder of that series differs

    # the digest covers the first 2 * length entries (the valid (value, mask) pairs): padding and what lies past the length do not
    # count, the mask does
    assert pc.token_idents(full, _series([a, a], 64), lengths, counts, TS0) == same
    c = np.concatenate([a, [5.0]])
    assert pc.token_idents(full, _series([a, c], 48), lengths, counts, TS0) == same
    masked = _series([a, a], 48)
    masked[1, 2 * 10 + 1, 0] = 0.0
    assert pc.token_idents(full, masked, lengths, counts, TS0)[6:9] != same[6:9]
    shorter = pc.token_idents(full, _series([a, a], 48), [40, 39], counts, TS0)
    assert shorter[2:5] == same[2:5] and shorter[6:9] != same[6:9]

    # host arrays digest like tensors; no series: only text tokens
    assert pc.token_idents(full, _series([a, a], 48).numpy(), lengths, counts, TS0) == same
    assert pc.token_idents([1, 2, 3], None, None, [], TS0) == [1, 2, 3]
