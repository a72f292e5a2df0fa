"""The byte layout of the weight arena, pinned to what another commit's library wrote (tests/golden/arena_layout.json,
scripts/gen_golden_arena_layout.py): the sha256 of the WHOLE arena — handed over zeroed, loaded with tensors that a closed formula fills —
after the load (every checkpoint slot, the SMPL block, the index tables, the padding rows, the flag words) and after finalize in the fp32
mode (repacked convs, codebook transpose, code norms, derived SMPL regions, encoder repacks).  The arena is broadcast between ranks byte
for byte: a slot that moved is a wrong model on every receiver."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_golden_arena_layout as AL      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", AL.GPU_CASES, ids=lambda c: c["name"])
def test_arena_bytes_are_pinned(built_lib, cuda_dev, case):
    with open(AL.GOLDEN) as f:
        golden = json.load(f)
    assert [{k: c[k] for k in case} for c in golden["device"]] == list(AL.GPU_CASES), "the fixture's cases are not the script's"
    assert (golden["vit_depth"], golden["dec_depth"], golden["max_batch"]) == (AL.VIT_DEPTH, AL.DEC_DEPTH, AL.MAX_BATCH)
    expect = next(c for c in golden["device"] if c["name"] == case["name"])
    got = AL.run_case(case, cuda_dev)
    print(case["name"], got)
    assert got["weight_bytes"] == expect["weight_bytes"]
    assert got["sha256_loaded"] == expect["sha256_loaded"], "the arena differs after load: a slot, the SMPL block, a table or a flag word moved"
    assert got["sha256_finalized"] == expect["sha256_finalized"], "the arena differs after finalize: a derived region moved or changed"
