"""Host-side detokenisation shared by the server and the engine: incremental text deltas and the stop-string rule.

The stop rule (vLLM's `stop=` / `include_stop_str_in_output=`, what the reference's drivers and its ReAct agent pass): with
`text(j)` the decode of the first j generated tokens (`skip_special_tokens=True`, a trailing U+FFFD - an incomplete multi-byte piece -
removed: it is not yet text), a sequence stops at the SMALLEST j for which `text(j)` contains a stop string; among the matches in that
text the one that starts first wins, ties go to the string listed first.  The returned text ends where the match starts (where it
ends with include_stop_str_in_output).  `StopChecker` evaluates exactly this, token by token over what a harvest brought - no shortcut
over several tokens, because `text(j)` need not be a prefix of `text(j + 1)` for every tokenizer.
"""

REPLACEMENT = "�"
MAX_STOP_STRINGS = 16


def stable_text(tokenizer, ids, final=False):
    """text(j) of the stop rule for ids = the first j tokens (final: the sequence is over, a trailing U+FFFD stays)"""
    full = tokenizer.decode(list(ids), skip_special_tokens=True)
    if not final and full.endswith(REPLACEMENT):
        full = full[:-1]
    return full


def normalize_stop(stop):
    """`stop` as callers pass it (None, a string, a list / tuple of strings) -> list of strings; ValueError for empty strings,
    non-strings and more than MAX_STOP_STRINGS entries."""
    if stop is None:
        return []
    if isinstance(stop, str):
        stop = [stop]
    if not isinstance(stop, (list, tuple)):
        raise ValueError(f"stop must be a string or a list of strings, got {type(stop).__name__}")
    out = []
    for s in stop:
        if not isinstance(s, str) or not s:
            raise ValueError(f"stop entries must be non-empty strings, got {s!r}")
        out.append(s)
    if len(out) > MAX_STOP_STRINGS:
        raise ValueError(f"at most {MAX_STOP_STRINGS} stop strings, got {len(out)}")
    return out


def find_stop(text, stops):
    """-> (start, stop string) of the match of the rule in `text`, or None"""
    best = None
    for s in stops:
        i = text.find(s)
        if i >= 0 and (best is None or i < best[0]):
            best = (i, s)
    return best


def held_back(text, stops):
    """length of the longest tail of `text` that is a proper prefix of a stop string (what a stream must not show yet)"""
    n = 0
    for s in stops:
        for k in range(min(len(s) - 1, len(text)), n, -1):
            if text.endswith(s[:k]):
                n = k
                break
    return n


class IncrementalDecoder:
    """token ids -> text deltas.  Decodes the whole sequence each time and emits the new suffix, holding back a trailing
    replacement character (an incomplete multi-byte piece), like vLLM's incremental detokenizer."""

    def __init__(self, tokenizer):
        self.tok, self.ids, self.text = tokenizer, [], ""

    def push(self, new_ids, final=False):
        self.ids += list(new_ids)
        full = stable_text(self.tok, self.ids, final)
        delta = full[len(self.text):] if full.startswith(self.text) else full
        self.text = full if full.startswith(self.text) else self.text + delta
        return delta


class StopChecker:
    """The stop rule over a growing token sequence.  push(new_ids) -> None, or (j, text, matched string): the sequence stops after
    its first j tokens with that final text.  `released` is the text a stream may show so far: text(j) without its held-back tail."""

    def __init__(self, tokenizer, stop, include_stop_str_in_output=False, min_tokens=0):
        self.tok, self.stops, self.include = tokenizer, normalize_stop(stop), bool(include_stop_str_in_output)
        self.ids, self.released, self.hit = [], "", None
        # min_tokens (vLLM's rule): no stop string is searched in the text the first min_tokens tokens produced - `base` characters
        self.min_tokens, self.base = max(0, int(min_tokens or 0)), 0

    def push(self, new_ids):
        if self.hit is not None:
            return self.hit
        for t in new_ids:
            self.ids.append(int(t))
            text = stable_text(self.tok, self.ids)
            if len(self.ids) <= self.min_tokens:
                self.base = len(text)
                self.released = text if text.startswith(self.released) else self.released
                continue
            m = find_stop(text[self.base:], self.stops) if self.base <= len(text) else None
            if m is not None:
                m = (m[0] + self.base,) + tuple(m[1:])
                end = m[0] + (len(m[1]) if self.include else 0)
                self.released = text[:end]
                self.hit = (len(self.ids), self.released, m[1])
                return self.hit
            shown = text[:len(text) - held_back(text, self.stops)]
            if shown.startswith(self.released):        # (a stream never takes text back)
                self.released = shown
        return None

    def finish(self, ids):
        """the sequence ended for another reason (EOS, a stop token, max_tokens) after `ids`: its final text, nothing held back"""
        self.ids = [int(t) for t in ids]
        self.released = stable_text(self.tok, self.ids, final=True)
        return self.released
