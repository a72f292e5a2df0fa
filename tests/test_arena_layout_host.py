"""The checkpoint contract and the arena sizes, pinned to what another commit's library reported (tests/golden/arena_layout.json,
scripts/gen_golden_arena_layout.py): thmr_spec name by name IN ORDER — spec order is arena order — thmr_arena_bytes and thmr_mode_bytes
in both modes, for three depths, both heads and two batch limits.  No device."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_golden_arena_layout as AL      # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(AL.GOLDEN) as f:
        return json.load(f)


def test_fixture_is_the_scripts(golden):
    assert [{k: c[k] for k in ("vit_depth", "dec_depth", "head", "max_batch")} for c in golden["host"]] == list(AL.HOST_CONFIGS)
    assert golden["commit"] and golden["src"].startswith("src:")
    assert all(len(c["spec"]) > 30 and c["weight_bytes"] > 0 and c["scratch_bytes"] > 0 for c in golden["host"])


@pytest.mark.parametrize("cfg", AL.HOST_CONFIGS, ids=lambda c: "{head}.v{vit_depth}.d{dec_depth}.b{max_batch}".format(**c))
def test_spec_and_sizes_are_pinned(built_lib, golden, cfg):
    expect = next(c for c in golden["host"] if all(c[k] == v for k, v in cfg.items()))
    got = AL.host_record(built_lib, **cfg)
    assert len(got["spec"]) == len(expect["spec"])
    for i, (g, x) in enumerate(zip(got["spec"], expect["spec"])):
        assert g == x, (i, g, x)
    for k in ("weight_bytes", "scratch_bytes", "mode_bytes"):
        assert got[k] == expect[k], (k, got[k], expect[k])
