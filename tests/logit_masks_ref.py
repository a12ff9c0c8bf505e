"""numpy float32 restatement of the logit masks pass (csrc/logit_masks.hip): allowed_token_ids -> logit_bias -> min_tokens on one row
of raw logits.  Only a copy of the bits, -inf and ONE float32 add per biased id are used, all of them exact, so a comparison with the
kernel is bitwise (NaN payloads included: an id without a bias is never passed through arithmetic)."""
import numpy as np

NEG_INF_BITS = np.uint32(0xFF800000)


def apply(row, allowed=None, bias=None, min_tokens=0, end_ids=(), step=0, vocab_offset=0):
    """row: float32 [V], the logits of global ids vocab_offset .. vocab_offset + V - 1.  allowed: iterable of global ids or None;
    bias: {global id: float} or None (distinct ids); end_ids: the ids kept away while step < min_tokens.  Ids outside the slice are
    skipped.  -> float32 [V] (a new array)"""
    row = np.ascontiguousarray(row, dtype=np.float32)
    V = row.shape[0]
    out = row.view(np.uint32).copy()
    if allowed is not None:
        keep = np.zeros(V, dtype=bool)
        idx = np.asarray(list(allowed), dtype=np.int64) - vocab_offset
        keep[idx[(idx >= 0) & (idx < V)]] = True
        out[~keep] = NEG_INF_BITS
    out = out.view(np.float32)
    for t, b in (bias or {}).items():
        i = int(t) - vocab_offset
        if 0 <= i < V:
            with np.errstate(invalid="ignore", over="ignore"):
                out[i] = np.float32(out[i]) + np.float32(b)
    if step < min_tokens:
        for t in end_ids:
            i = int(t) - vocab_offset
            if 0 <= i < V:
                out[i] = -np.inf
    return out


def bitset(allowed, n_words):
    """allowed global ids -> uint32 [n_words]: bit of id i = word i // 32, bit i % 32"""
    bits = np.zeros(n_words, dtype=np.uint32)
    ids = np.asarray(list(allowed), dtype=np.int64)
    np.bitwise_or.at(bits, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return bits


def argmax(row):
    """the selection's greedy rule on a processed row: the largest logit, the lowest id among equals (NaN never wins)"""
    r = np.where(np.isnan(row), -np.inf, row.astype(np.float64))
    return int(np.argmax(r))
