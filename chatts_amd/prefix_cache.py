"""Prefix reuse between KV cache slots (vLLM's enable_prefix_caching): which tokens are the same, which slot a request should take
and how much of its prompt is already resident.  Plain host arithmetic on lists of token identities; the model owns the slots'
identity lists (ChatTSForCausalLM._slot_idents) and does the copying / block sharing."""
import hashlib

import numpy as np

MIN_REUSE = 16          # tokens: a shorter common prefix is not worth a copy + a ragged prefill start


def token_idents(full, series, lengths, counts, ts0):
    """Identity of every token of an EXPANDED prompt: the id for text tokens; for a <ts> placeholder the digest of its
    series' (value, mask) row + the patch index - two placeholder rows hold the same embedding iff those agree."""
    digests = []
    if series is not None and len(counts):
        host = series.detach().cpu().numpy() if hasattr(series, "detach") else np.asarray(series)
        for i, L in enumerate(lengths):
            digests.append(hashlib.blake2b(np.ascontiguousarray(host[i].reshape(-1)[:2 * int(L)]).tobytes(), digest_size=8).digest())
    placeholders = [(digests[i], p) for i, c in enumerate(counts) for p in range(int(c))]     # in prompt order
    out, j = [], 0
    for t in full:
        if t == ts0:
            out.append(placeholders[j])
            j += 1
        else:
            out.append(t)
    return out


def common_prefix_len(a, b):
    n = 0
    for x, y in zip(a, b):
        if x != y:
            break
        n += 1
    return n


def match_prefix(slot_idents, idents, slot, exclude=()):
    """(n, src): the longest prefix of `idents` resident in some cache slot (ties prefer `slot` itself: zero copy); (0, -1) for none."""
    best, src = 0, -1
    for s, have in enumerate(slot_idents):
        if s in exclude:
            continue
        n = common_prefix_len(idents, have)
        if n > best or (n == best and s == slot and n > 0):
            best, src = n, s
    return best, src


def pick_slot(slot_idents, free_slots, idents):
    """The free slot whose resident prefix matches `idents` best when that match is worth reusing (zero copy), else the one whose
    resident tokens are least worth keeping (fewest)."""
    best = max(free_slots, key=lambda s: common_prefix_len(idents, slot_idents[s]))
    if common_prefix_len(idents, slot_idents[best]) >= MIN_REUSE:
        return best
    return min(free_slots, key=lambda s: len(slot_idents[s]))
