"""Call trace of the Python `split_epoch` loop on the GPU (`--python_epoch --split_persist off`),
where Bob's tail has its fused (vanilla `train_fwd_bwd3` / `fused_step`) and grouped (U-shape
`group_step`) kernels, the head is one `head_step` launch and the look-ahead order passes the
next batch's activation into Bob's update: the branches tests/test_split_trace_cpu.py cannot
reach.  Same recorder, same four cases, 37 samples at B = 16.

The expected traces are tests/data/split_epoch_trace_gpu.json, regenerated only by hand on a
GPU machine: `python -m tests.test_split_trace_cpu --gpu`.
"""
import json
import os

import pytest

from test_split_trace_cpu import CASES, DATA, case_id, record_trace

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind,ahead", CASES)
def test_split_epoch_call_trace_gpu(cuda, kind, ahead, tmp_path):
    with open(os.path.join(DATA, "split_epoch_trace_gpu.json")) as f:
        want = json.load(f)[case_id(kind, ahead)]
    got = json.loads(json.dumps(record_trace(kind, ahead, tmp_path, cuda,
                                             ("--python_epoch", "--split_persist", "off"))))
    assert len(got) > 20
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
    assert len(got) == len(want)
