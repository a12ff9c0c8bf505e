"""The decoder schedule's pass state must not leak from one entry point into the next: the reduced stage list of
tools/decoder_schedule_ab.py runs twice in one process on the same model objects and every digest of round 2 must equal round 1 bit
for bit; the decode tokens must be the float32 oracle's (the check of test_gpu_e2e.py::test_generate_matches_oracle).  No recorded
digests: those would pin today's kernels."""
import importlib.util
import os

import pytest

from chatts_amd import synth
from oracle import pipeline, synth as osynth

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "decoder_schedule_ab", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "decoder_schedule_ab.py"))
ab = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ab)


def test_round2_equals_round1_and_decode_matches_oracle():
    res = ab.run("tiny-qwen2", "f32", ab.REDUCED, rounds=2)
    first, second = res["rounds"]
    assert {name for name, *_ in ab.REDUCED} == {k.split("/")[2] for k in first}            # every stage reported
    assert first.keys() == second.keys()
    assert [k for k in first if second[k] != first[k]] == []
    assert res["differs"] == []
    cfg, ids, ts = res["request"]
    tokens = first["tiny-qwen2/f32/decode4/tokens"]
    assert len(tokens) == 5                                                                   # the first token + 4 decode steps
    sd = osynth.state_dict(synth.all_specs(cfg), 3)
    want = pipeline.generate(cfg, sd, ids, ts.numpy(), len(tokens))
    assert tokens == want["tokens"]
    assert second["tiny-qwen2/f32/decode4/tokens"] == want["tokens"]
