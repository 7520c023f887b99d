"""The host-side derivation of the int8 fixed-point epilogue (csrc/y355_requant.h), pinned to tests/golden/requant_parent.json:
tests/requant_host_check.cpp, built with plain g++, prints for every case of its sweep what the header derives -- return code and
message, every field of every struct, CRCs of the bias and shift vectors -- and every line equals (by its CRC-32) what the parent commit's
statements (make_requant of engine.hip; conv_fixed, fits32, res_params and the rule blocks of refresh_layer_i8 / cal_conv_max of
net.hip) answered for that case (tests/golden/gen_golden_requant.py says how that was recorded).  The recording reaches every
case the rules distinguish, and int8_tile_cases.narrow_rule, the same rule in exact rationals, agrees with `narrow` on every
y355_net record.  Needs no GPU and no built library."""
import importlib.util
import json
import os
import subprocess

import pytest

import int8_tile_cases as TC

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
_spec = importlib.util.spec_from_file_location("gen_golden_requant", os.path.join(GOLDEN, "gen_golden_requant.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)                               # the line format and the list of cases: one definition

with open(os.path.join(GOLDEN, "requant_parent.json")) as _f:
    DOC = json.load(_f)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("requant") / "requant_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", os.path.join(HERE, "requant_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_every_line_is_the_parents(lines):
    want = " ".join(DOC["crc32"]).split()
    assert len(DOC["parent"]) == 40 and 2000 <= len(want) <= 5000 and len(want) == DOC["lines"]
    assert len(lines) == len(want)
    bad = [(i, l) for i, (l, w) in enumerate(zip(lines, want)) if G.crc(l) != w]
    assert not bad, bad[:5]


def test_the_recording_reaches_every_case(lines):
    """the parent's own lines reached every case (counted when they were recorded), and so do this program's"""
    for cov in (DOC["coverage"], G.coverage(lines)):
        assert not G.missing(cov), G.missing(cov)
        # the engine's clamp of sh to 31 when not wide cannot fire: sh > 31 adds 2^(sh - 1) >= 2^31 to the bound, which makes the
        # layer wide.  Its input range is reached, and the shift stays as asked there
        assert cov["engine sh clamped to 31"] == 0 and cov["engine sh 32 .. 62 is wide, unclamped"] > 0
    assert DOC["coverage"] == G.coverage(lines)


def test_the_rational_rule_agrees_on_every_net_record(lines):
    """narrow_rule knows only the layer's own weights: where the sums |q_w| are unknown (all zero) the C bound is 127 per
    weight, which is sum |q_w| = 127 K in every channel"""
    n = 0
    for r in map(G.parse, lines):
        if r["what"] != "N" or r["fixed_rc"] or r["rc"]:
            continue
        K = r["ksize"] * r["ksize"] * r["cin"]
        wabs = r["wabs"] if max(r["wabs"]) > 0 else [127 * K] * r["cout"]
        got = TC.narrow_rule(r["sa_i"], r["e_wc"], r["e_b"], max(abs(b) for b in r["q_b"]), wabs, r["lk"], r["nm"], r["sa_o"],
                             r["s_r"] if r["kind"] == 4 else None)
        assert got == bool(r["rq"]["narrow"]), r
        n += 1
    assert n > 400
