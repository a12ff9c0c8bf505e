"""numpy / plain-Python references of prompt-lookup speculative decoding (csrc/spec_decode.hip): the proposer rule in its two
formulations, the accept rule of chatts_spec_verify, and a simulator of a whole generation.  TEST INFRASTRUCTURE ONLY."""
import numpy as np


def propose_by_match_length(hist, pos, k, ngram_min, ngram_max):
    """The rule as chatts_amd.h states it.  Context hist[0 .. pos]; for a candidate end e < pos, m(e) = the largest m <= ngram_max
    with hist[e - j] == hist[pos - j] for all j < m; the e with the largest m(e) >= ngram_min wins, ties to the smallest e.
    -> (drafts [k] with -1 fill, e or None)"""
    best_m, best_e = 0, None
    for e in range(pos):
        m = 0
        while m < ngram_max and e - m >= 0 and hist[e - m] == hist[pos - m]:
            m += 1
        if m >= ngram_min and m > best_m:
            best_m, best_e = m, e
    return _drafts(hist, pos, k, best_e), best_e


def propose_by_ngram_search(hist, pos, k, ngram_min, ngram_max):
    """The same rule the way vLLM / HF describe it: for n from ngram_max down to ngram_min, the earliest earlier occurrence of the
    last n tokens that has at least one token after it."""
    for n in range(ngram_max, ngram_min - 1, -1):
        if n > pos + 1:
            continue
        tail = list(hist[pos - n + 1:pos + 1])
        for e in range(n - 1, pos):                     # the occurrence ends at e < pos: hist[e + 1] exists
            if list(hist[e - n + 1:e + 1]) == tail:
                return _drafts(hist, pos, k, e), e
    return [-1] * k, None


def _drafts(hist, pos, k, e):
    if e is None:
        return [-1] * k
    return [int(hist[e + 1 + j]) if e + 1 + j <= pos else -1 for j in range(k)]


def spec_tokens(hist, pos, drafts, vocab):
    """the step's input ids: the last token, then the drafts with invalid ones replaced by id 0"""
    return [int(hist[pos])] + [d if 0 <= d < vocab else 0 for d in drafts]


def verify(argmax, drafts, pos, step, out_capacity, max_ctx, vocab):
    """chatts_spec_verify -> dict(e, valid, appended tokens, new pos / step / token, counter increments) or None (nothing happens)"""
    k = len(drafts)
    a = 0
    while a < k and 0 <= drafts[a] < vocab and drafts[a] == argmax[a]:
        a += 1
    valid = sum(1 for d in drafts if 0 <= d < vocab)
    e = min(a + 1, out_capacity - step, max_ctx - (k + 1) - pos)
    if e <= 0 or pos < 0 or step < 0:
        return None
    return dict(e=e, a=a, valid=valid, tokens=[int(t) for t in argmax[:e]], pos=pos + e, step=step + e, token=int(argmax[e - 1]),
                counters=(1, valid, e - 1, e))


def simulate(prompt_ids, tokens, k, ngram_min, ngram_max):
    """Greedy generation whose result is `tokens` (token 0 comes from the prefill), replayed with speculative steps: every step
    proposes from the context so far, accepts the drafts that equal the true continuation and emits one more token, never past
    len(tokens).  -> (accept count per step, counters dict)"""
    hist = list(prompt_ids) + [tokens[0]]
    done, accepts = 1, []
    drafted = 0
    while done < len(tokens):
        pos = len(hist) - 1
        drafts, _ = propose_by_match_length(hist, pos, k, ngram_min, ngram_max)
        drafted += sum(1 for d in drafts if d >= 0)
        a = 0
        while a < k and drafts[a] >= 0 and done + a < len(tokens) and drafts[a] == tokens[done + a]:
            a += 1
        e = min(a + 1, len(tokens) - done)
        accepts.append(e - 1)
        hist += list(tokens[done:done + e])
        done += e
    return accepts, dict(steps=len(accepts), drafted=drafted, accepted=int(np.sum(accepts)) if accepts else 0, emitted=len(tokens) - 1)
