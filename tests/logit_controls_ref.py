"""CPU restatement (numpy float64) of the logit controls of csrc/logit_controls.hip, in vLLM V1's sampler order:
raw logits -> repetition -> frequency and presence -> [greedy rows: argmax of these] -> temperature -> min_p -> top-k -> top-p -> draw.

  repetition r   every id that occurs in the prompt or among the generated tokens: l / r if l > 0 else l * r
  frequency f    l -= f * c, c = occurrences of the id among the GENERATED tokens so far
  presence p     l -= p if c > 0
  min_p          (sampled rows) id i survives iff l_i >= m + T * log(min_p), m the row maximum of the penalised logits; ties are kept
"""
import numpy as np

from oracle import sampler as osampler

EPS = 2.0 ** -24            # half an ulp of a float32 of magnitude < 1, relative


def counts_of(generated, vocab, vocab_offset=0):
    """occurrences of every id of the slice [vocab_offset, vocab_offset + vocab) among `generated` (global ids)"""
    g = np.asarray(list(generated), dtype=np.int64) - vocab_offset
    g = g[(g >= 0) & (g < vocab)]
    return np.bincount(g, minlength=vocab).astype(np.int64)


def prompt_mask(prompt, vocab, vocab_offset=0):
    m = np.zeros(vocab, dtype=bool)
    p = np.asarray(list(prompt), dtype=np.int64) - vocab_offset
    m[p[(p >= 0) & (p < vocab)]] = True
    return m


def penalise(logits, in_prompt, counts, r=1.0, f=0.0, p=0.0):
    """float64 penalised logits of one row"""
    l = np.asarray(logits, dtype=np.float64).copy()
    c = np.asarray(counts, dtype=np.float64)
    seen = np.asarray(in_prompt, dtype=bool) | (c > 0)
    l[seen] = np.where(l[seen] > 0, l[seen] / r, l[seen] * r)
    l = l - f * c
    l[c > 0] -= p
    return l


def penalty_bound(logits, counts, r=1.0, f=0.0, p=0.0):
    """|float32 kernel - float64 reference| per id: at most four float32 roundings (quotient or product, f * c, two subtractions),
    each at most half an ulp of a magnitude bounded by the sum"""
    l = np.abs(np.asarray(logits, dtype=np.float64))
    l = np.where(np.isfinite(l), l, 0.0)
    return 4 * EPS * (l * max(r, 1.0 / r) + abs(f) * np.asarray(counts, dtype=np.float64) + abs(p))


def min_p_cut(pen, temperature, min_p):
    """the cut of one row (None when min_p is inert: off, or a greedy row)"""
    if not (min_p > 0.0 and temperature > 0.0):
        return None
    fin = pen[~np.isnan(pen)]
    return float(fin.max()) + temperature * np.log(min_p)


def apply(logits, in_prompt, counts, r=1.0, f=0.0, p=0.0, min_p=0.0, temperature=0.0):
    """-> (float64 logits the selection sees: penalised, ids below the min_p cut at -inf; the cut or None)"""
    pen = penalise(logits, in_prompt, counts, r, f, p)
    cut = min_p_cut(pen, temperature, min_p)
    if cut is not None:
        pen = np.where(pen >= cut, pen, -np.inf)
    return pen, cut


def greedy(logits, in_prompt, counts, r=1.0, f=0.0, p=0.0):
    """(token, margin between the two best penalised logits)"""
    pen = penalise(logits, in_prompt, counts, r, f, p)
    tok = int(np.argmax(pen))
    top2 = np.partition(pen, -2)[-2:]
    return tok, float(top2[1] - top2[0])


def sample(logits, in_prompt, counts, temperature, top_k, top_p, seed, step, r=1.0, f=0.0, p=0.0, min_p=0.0, seq=0):
    """the token the per-row sampler draws from the controlled logits (oracle.sampler's rule and variate)"""
    sel, _ = apply(logits, in_prompt, counts, r, f, p, min_p, temperature)
    return osampler.sample(sel.astype(np.float32), temperature, top_k, top_p, seed, seq, step)
