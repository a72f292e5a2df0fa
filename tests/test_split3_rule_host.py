"""The split3 GEMM's tile rule (tokenhmr_amd/csrc/gemm_split3_rule.h) without a device: a plain C++ program that includes that header
ALONE prints split3_rule::choose's answer for a table of cases — the engine's shapes over the batch sizes at which the answer changes, and
the edges of every condition — and the answers are compared with what the launchers did before the rule was a function of its own
(launch_split3_tiles + launch_split16_tiles_tail, read line by line).  Also: every knob of the rule is read in ONE file of csrc/."""
import glob
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tokenhmr_amd", "csrc")
NONE, BIAS, GELU, RESID, QSCALE, POS = 0, 1, 2, 4, 5, 6          # common.h GemmEpi

# answers, as the program prints them
S3 = "tiles 3"              # 128 x 128, four waves, three-stage K ring (variant 8)
FRONT = "tiles 5"           # 128 x 256 with front-loaded copies (variant 10)
PLAIN = "tiles 0"           # 128 x 256
REFUSE = "refuse"


def tail(q, tail_from, tail8=0):
    return f"tail {q} {tail_from} {tail8}"


def case(M, N, ksplit=1, a_blk=0, epi=NONE, variant=-1, opts=0, cus=256):
    return (M, N, ksplit, a_blk, epi, variant, opts, cus)


def engine_cases():
    """(B, GEMM) -> answer on 256 compute units with no option bit: M = 192 B; qkv N = 3840, fc1 N = 5120, proj / fc2 N = 1280 with the
    plan's split factors (vit_plan.h: four ways at 3-4 crops, two ways at 5-15, fc2 two ways up to 31)."""
    out = {}

    def put(B, qkv, proj, fc1, fc2):
        ks_proj = 4 if B < 5 else 2 if B < 16 else 1
        ks_fc2 = 4 if B < 5 else 2 if B < 32 else 1
        M = 192 * B
        out[f"b{B}.qkv"] = (case(M, 3840, epi=QSCALE), qkv)
        out[f"b{B}.proj"] = (case(M, 1280, ks_proj, epi=NONE if ks_proj > 1 else RESID), proj)
        out[f"b{B}.fc1"] = (case(M, 5120, epi=GELU), fc1)
        out[f"b{B}.fc2"] = (case(M, 1280, ks_fc2, epi=NONE if ks_fc2 > 1 else RESID), fc2)

    for B in (3, 4):
        put(B, S3, S3, S3, S3)
    put(5, S3, S3, FRONT, S3)
    put(8, FRONT, S3, FRONT, S3)
    put(15, FRONT, FRONT, FRONT, FRONT)
    put(16, tail(45, 32), S3, FRONT, FRONT)
    put(17, FRONT, FRONT, tail(65, 64), FRONT)
    for B in (24, 32, 33, 40):
        put(B, PLAIN, FRONT, PLAIN, FRONT)
    put(48, tail(135, 128), tail(45, 32), PLAIN, tail(45, 32))
    put(64, PLAIN, FRONT, tail(240, 224), FRONT)
    put(128, tail(360, 352), PLAIN, PLAIN, PLAIN)
    return out


EDGES = {
    "a_blk.fc2.b64": (case(12288, 1280, a_blk=1, epi=RESID), PLAIN),                  # a row-blocked A is never front-loaded
    "patch_embed.b48": (case(9216, 1280, epi=POS), FRONT),                            # q = 45 would qualify: the tail kernel has no such epilogue
    "cus304": (case(12288, 5120, cus=304), tail(240, 228)),
    "cus8": (case(12288, 5120, cus=8), PLAIN),
    "t128.256": (case(2048, 2048), S3),                                               # exactly one round of 128 x 128 tiles
    "t128.272": (case(2049, 2048), FRONT),
    "opts0": (case(768, 5120, opts=0), "tiles 3"),                                    # ids 8 / 9 / 2 / 6
    "opts1": (case(768, 5120, opts=1), "tiles 4"),
    "opts4": (case(768, 5120, opts=4), "tiles 1"),
    "opts5": (case(768, 5120, opts=5), "tiles 2"),
    "tail8.bit": (case(12288, 5120, opts=2), tail(240, 224, 1)),
    "front.off": (case(6144, 1280, opts=8), PLAIN),
    "front.on": (case(6144, 1280), FRONT),
    "id5.no_tail": (case(6144, 1280, variant=5), REFUSE),
    "tail.off": (case(12288, 5120, epi=GELU, opts=16), PLAIN),
    # beyond the issue's table, from the same reading of the launchers
    "id5": (case(12288, 5120, variant=5), tail(240, 224)),
    "id7": (case(12288, 5120, variant=7), tail(240, 224, 1)),
    "id5.tail.off": (case(12288, 5120, variant=5, opts=16), tail(240, 224)),         # asked for explicitly: the switch does not apply
    "id5.pos": (case(9216, 1280, epi=POS, variant=5), REFUSE),
    "id5.ksplit": (case(12288, 5120, ksplit=2, variant=5), REFUSE),
    "id0": (case(12288, 5120, variant=0), PLAIN),                                     # an explicit 128 x 256: neither tail nor front
    "id0.small": (case(768, 5120, variant=0), PLAIN),
    "id10": (case(12288, 5120, variant=10), FRONT),
    "id11": (case(768, 5120, variant=11), "tiles 6"),
    "id2.big": (case(12288, 5120, variant=2), "tiles 1"),
    "exp20": (case(12288, 5120, variant=20), "exp 20"),
    "exp37": (case(768, 1280, variant=37), "exp 37"),
    "a_blk.bias": (case(12288, 1280, a_blk=1, epi=BIAS), REFUSE),
    "a_blk.bias.exp": (case(12288, 1280, a_blk=1, epi=BIAS, variant=20), REFUSE),
    "a_blk.tail": (case(9216, 1280, a_blk=1, epi=RESID), tail(45, 32)),
    "a_blk.none.small": (case(768, 1280, 4, a_blk=1), S3),
    "ksplit.no_tail": (case(9216, 1280, 2), PLAIN),                                   # 720 > 512 units, and split K never takes the tail
    "front.512": (case(128 * 128, 1024), FRONT),                                      # 128 x 4 = 512 tiles; q = 64 = two whole rounds: no tail
    "front.513": (case(128 * 171, 768), PLAIN),                                       # 171 x 3 = 513 tiles (513 % 8 != 0: no tail)
    "tail.rem.half": (case(128 * 96, 1024), tail(48, 32)),                            # rem = 16 = per / 2: the last one that qualifies
    "tail.rem.over": (case(128 * 98, 1024), FRONT),                                   # q = 49, rem = 17
    "tail.one_round": (case(128 * 36, 1024), FRONT),                                  # q = 18 < per: less than one whole round
    "cus.odd": (case(12288, 5120, cus=250), PLAIN),                                   # cus % 8 != 0
    "n.ragged": (case(12288, 5000), PLAIN),                                           # N % 256 != 0
}


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    import __graft_entry__
    cases = {**engine_cases(), **EDGES}
    d = tmp_path_factory.mktemp("split3_rule")
    lines = ['#include "gemm_split3_rule.h"', "#include <cstdio>", "using namespace split3_rule;",
             "static void show(const char* name, Choice c) {",
             '    if (c.kind == Choice::REFUSE) printf("%s refuse\\n", name);',
             '    else if (c.kind == Choice::TILES) printf("%s tiles %d\\n", name, c.shape);',
             '    else if (c.kind == Choice::TAIL) printf("%s tail %d %d %d\\n", name, c.q, c.tail_from, (int)c.tail8);',
             '    else printf("%s exp %d\\n", name, c.shape);', "}", "int main() {"]
    lines += [f'    show("{name}", choose({", ".join(str(int(v)) for v in args)}));' for name, (args, _) in cases.items()]
    (d / "rule.cpp").write_text("\n".join(lines + ["    return 0;", "}"]) + "\n")
    r = subprocess.run([__graft_entry__._hipcc(), "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(d / "rule.cpp"), "-o", str(d / "rule")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    out = subprocess.run([str(d / "rule")], capture_output=True, text=True, check=True).stdout.splitlines()
    got = dict(line.split(" ", 1) for line in out)
    assert set(got) == set(cases)
    return cases, got


def test_rule_header_includes_nothing():
    text = open(os.path.join(CSRC, "gemm_split3_rule.h")).read()
    assert not re.findall(r"^\s*#\s*include", text, flags=re.M)


def test_engine_shapes(answers):
    cases, got = answers
    wrong = {n: (got[n], want) for n, (_, want) in cases.items() if n.startswith("b") and got[n] != want}
    assert not wrong, wrong
    assert sum(n.startswith("b") for n in cases) == 4 * 14


def test_edges(answers):
    cases, got = answers
    wrong = {n: (got[n], want) for n, (_, want) in cases.items() if not n.startswith("b") and got[n] != want}
    assert not wrong, wrong


def test_each_tile_knob_is_read_in_one_file():
    texts = {f: open(f).read() for f in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))}
    for knob in ("THMR_SPLIT3_TILE", "THMR_SPLIT3_NARROW8", "THMR_SPLIT3_TAIL8", "THMR_SPLIT3_RING3", "THMR_SPLIT3_FRONT", "THMR_SPLIT3_TAIL"):
        files = [os.path.basename(f) for f, t in texts.items() if re.search(r"\b%s\b" % knob, t)]
        assert files == ["gemm_split3_dispatch.hip"], (knob, files)
