"""TEST INFRASTRUCTURE -- tests/golden/requant_parent.json: what the host-side derivation of the int8 fixed-point epilogue
answered at the commit named in the file, BEFORE it moved into csrc/y355_requant.h, on the sweep of
tests/requant_host_check.cpp.  tests/test_requant_parent.py compares that program's lines with the recording.

How the recording was made.  The lines do not come from y355_requant.h: a scratch recorder (not committed) was built in a
checkout of the parent commit from
  * tests/requant_host_check.cpp of this commit with two parts replaced: the include of y355_requant.h, and the four functions
    between "the code under test" and "printing" (run_engine, run_fixed, run_refresh, run_stat) -- the sweep and the printing
    are this commit's, so both programs print the same cases in the same format;
  * the parent's statements, lifted unedited by line range: csrc/y355_common.h:25-60 and :488-507 (Requant, the fp32 rules,
    RequantG, ResQ), csrc/engine.hip:111-165 (make_requant), csrc/net.hip:421-511 (act_fixed, acc_bound, ConvFixed, conv_fixed,
    fits32, requant_of, res_params), :578-639 (refresh_layer_i8, whole) and :1144-1163 (cal_conv_max up to its uploads);
  * stand-ins for what those statements touch: y355_fail keeping the message, HIPCHK / hipMemcpyAsync as a host memcpy into
    buffers the recorder reads back (the 32-bit biases of conv1.hip and front.hip), y355_pc_word, and a y355_net / NLayer /
    OpDef holding only the fields read, filled as load_layer_i8 fills them (e_w the largest exponent, pc, wabs).
  run_engine called make_requant; run_fixed conv_fixed; run_refresh refresh_layer_i8 on op 0 (first layer; front_graph for
  kind 2), op 1 (kind 3) or op 5; run_stat the lifted block of cal_conv_max.
Then:  recorder > lines.txt;  python tests/golden/gen_golden_requant.py <parent hash> lines.txt
which refuses to write a recording that misses one of the cases coverage() names.  The file keeps, per line of the parent's
output and in the sweep's order, the CRC-32 of the line ("crc32": rows of sixteen), and how many of the parent's lines reached
each case ("coverage"): the program prints the inputs with the outputs, so a line of equal CRC is the parent's line, and a
line that differs is shown by the test with its number.

A line (all integers unless said):
  E taps cin sa_in e_w e_b sa_out have_out act retune wabs cout cout_pad q_b[0] | rc ["message"] | R <Requant> frac_bits crc(bias_t) crc(bias_w)
  N kind ksize cin cout cout_pad sa_i e_b lk nm sa_o s_r ew_mode e <e_wc> w <wabs> b <q_b>
      | rc ["message"] or 0 F shl bshl E bmax tw tb (C hex floats) crc(bw) crc(shc)                      y355_rq_fixed
      | rc ["message"] or 0 G <RequantG> [Q <ResQ>] [R <Requant> crc(bt)] [R <Requant> crc(fb)]           a forward's refresh
      | rc ["message"] or 0 G <RequantG> R <Requant> Q <ResQ> frac_bits                                    the statistics pass
  <Requant> = its 15 fields in declaration order, then y355_fp32_slope_ok, y355_fp32_exact, y355_fp32_fold.
"""
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
RQ = ("shl", "sh", "leaky", "guard_log2", "wide", "lk", "sh_l", "sh_r", "hm1", "bw", "neg_mul", "gen32", "tmax_log2", "split", "negsafe",
      "slope_ok", "exact", "fold")
RG = ("shl", "sh", "lk", "neg_mul", "narrow", "split")
RR = ("t_sh", "r_sh", "sh", "p_t", "p_r", "p_d", "n_t", "n_r", "n_d")
E_IN = ("taps", "cin", "sa_in", "e_w", "e_b", "sa_out", "have_out", "act", "retune", "wabs", "cout", "cout_pad", "qb0")
N_IN = ("kind", "ksize", "cin", "cout", "cout_pad", "sa_i", "e_b", "lk", "nm", "sa_o", "s_r", "ew_mode")
GAP = "exponent gap too large for the fixed-point epilogue"
B62 = "fixed-point epilogue exceeds 62 bits"


def _section(text):
    """'rc "message"' or '0 tokens ...' -> (rc, message, tokens)"""
    rc, _, rest = text.partition(" ")
    if int(rc):
        assert rest.startswith('"') and rest.endswith('"'), text
        return int(rc), rest[1:-1], []
    return 0, "", rest.split()


def _take(tok, tag, names):
    assert tok[0] == tag, tok
    return dict(zip(names, map(int, tok[1:1 + len(names)]))), tok[1 + len(names):]


def parse(line):
    """one line of the program -> a dict (see the module's docstring)"""
    parts = line.split(" | ")
    head = parts[0].split()
    if head[0] == "E":
        d = dict(zip(E_IN, map(int, head[1:])), what="E")
        d["rc"], d["msg"], tok = _section(parts[1])
        if not d["rc"]:
            d["rq"], tok = _take(tok, "R", RQ)
            d["frac_bits"] = int(tok[0])
        return d
    assert head[0] == "N" and len(parts) in (2, 4), line
    d = dict(zip(N_IN, map(int, head[1:13])), what="N")
    n = d["cout"]
    assert head[13] == "e" and head[14 + n] == "w" and head[15 + 2 * n] == "b"
    d["e_wc"] = [int(v) for v in head[14:14 + n]]
    d["wabs"] = [int(v) for v in head[15 + n:15 + 2 * n]]
    d["q_b"] = [int(v) for v in head[16 + 2 * n:16 + 3 * n]]
    d["fixed_rc"], d["fixed_msg"], tok = _section(parts[1])
    if d["fixed_rc"]:
        return d
    d["F"], d["shl"], d["bshl"], d["E"] = map(int, tok[:4])
    d["rc"], d["msg"], tok = _section(parts[2])
    if not d["rc"]:
        d["rq"], tok = _take(tok, "G", RG)
        if d["kind"] == 4:
            d["rr"], tok = _take(tok, "Q", RR)
        if d["kind"] in (1, 2):
            d["rq1"], tok = _take(tok, "R", RQ)
            tok = tok[1:]
        if d["kind"] in (2, 3):
            d["fr"], tok = _take(tok, "R", RQ)
    d["stat_rc"], d["stat_msg"], _ = _section(parts[3])
    return d


def coverage(lines):
    """the cases the sweep has to reach -> how many lines reach each"""
    rec = [parse(l) for l in lines]
    E = [r for r in rec if r["what"] == "E"]
    Eok = [r for r in E if not r["rc"]]
    N = [r for r in rec if r["what"] == "N"]
    Nfx = [r for r in N if not r["fixed_rc"]]
    Nok = [r for r in Nfx if not r["rc"]]
    asked = lambda r: max(r["sa_in"] + r["e_w"], r["e_b"]) + (3 if r["act"] == 1 else 0) - r["sa_out"]      # F' - sa_out
    spread = lambda r: max(r["e_wc"]) - min(r["e_wc"])
    c = {}
    count = lambda name, rows: c.__setitem__(name, sum(1 for _ in rows))
    # engine / operator: every refusal of make_requant
    for name, msg in (("gap", GAP), ("output exponent", "output exponent too large"), ("62 bits", B62)):
        count("engine refuses: " + name, (r for r in E if r["rc"] == -4 and r["msg"] == msg))
    for f in ("wide", "negsafe", "exact"):
        for v in (0, 1):
            count("engine %s %d" % (f, v), (r for r in Eok if r["rq"][f] == v))
    for v in (0, 1, 2):
        count("engine FOLD %d" % v, (r for r in Eok if r["rq"]["fold"] == v))
        count("engine act %d" % v, (r for r in Eok if r["act"] == v))
    count("engine sh < 0", (r for r in Eok if r["rq"]["sh"] < 0))
    count("engine sh == 0", (r for r in Eok if r["rq"]["sh"] == 0 and r["have_out"]))
    count("engine sh > 0", (r for r in Eok if r["rq"]["sh"] > 0))
    count("engine sh clamped to 62", (r for r in Eok if r["have_out"] and asked(r) > 62 and r["rq"]["sh"] == 62))
    # `if (!wide && sh > 31) sh = 31` cannot fire: sh > 31 puts the rounding add 2^(sh - 1) >= 2^31 into the bound, which is
    # wide.  What can be reached is its input range, and that the shift then stays as asked
    count("engine sh 32 .. 62 is wide, unclamped", (r for r in Eok if r["have_out"] and 32 <= asked(r) <= 62 and r["rq"]["wide"] == 1 and r["rq"]["sh"] == asked(r)))
    count("engine sh clamped to 31", (r for r in Eok if r["have_out"] and asked(r) > 31 and r["rq"]["sh"] == 31))
    count("engine have_out 0", (r for r in Eok if not r["have_out"]))
    for v in (10, 11):
        count("engine retune %d" % v, (r for r in Eok if r["retune"] == v))
    count("engine wabs known", (r for r in Eok if r["wabs"] > 0))
    count("engine wabs unknown", (r for r in Eok if r["wabs"] == 0))
    for v in (1, 9, 25):
        count("engine taps %d" % v, (r for r in Eok if r["taps"] == v))
    # y355_net
    count("net refuses: gap (exponents in front)", (r for r in N if r["fixed_rc"] == -4 and r["fixed_msg"] == GAP))
    count("net refuses: gap (output exponent)", (r for r in Nfx if r["rc"] == -4 and r["msg"] == GAP))
    count("net refuses: 62 bits", (r for r in Nfx if r["rc"] == -4 and r["msg"] == B62))
    count("statistics pass refuses: 62 bits", (r for r in Nfx if r["stat_rc"] == -4 and r["stat_msg"] == B62))
    count("statistics pass refuses: residual gap", (r for r in Nfx if r["stat_rc"] == -4 and r["stat_msg"] == "residual layer: exponent gap too large"))
    for name, lk, nm in (("none", 0, 1), ("0.125", 3, 1), ("0.1", 11, 205)):
        count("net act " + name, (r for r in Nok if (r["lk"], r["nm"]) == (lk, nm)))
    count("net per-tensor exponent", (r for r in Nok if r["ew_mode"] == 0))
    count("net per-channel exponents, spread 0", (r for r in Nok if r["ew_mode"] == 1 and spread(r) == 0))
    count("net per-channel exponents, spread > 0", (r for r in Nok if r["ew_mode"] == 1 and spread(r) > 0))
    plain = [r for r in Nok if r["kind"] != 4]
    count("net narrow by fits32", (r for r in plain if r["rq"]["narrow"] and not r["rq"]["split"]))
    count("net narrow by split", (r for r in plain if r["rq"]["narrow"] and r["rq"]["split"]))
    count("net not narrow", (r for r in plain if not r["rq"]["narrow"]))
    for v in (0, 1):
        count("first layer gen32 %d" % v, (r for r in Nok if "rq1" in r and r["rq1"]["gen32"] == v))
        count("front form wide %d" % v, (r for r in Nok if "fr" in r and r["fr"]["wide"] == v))
        count("residual narrow %d" % v, (r for r in Nok if r["kind"] == 4 and r["rq"]["narrow"] == v))
    count("residual 62-bit refusal", (r for r in Nfx if r["kind"] == 4 and r["rc"] == -4 and r["msg"] == "residual epilogue exceeds 62 bits"))
    return c


UNREACHABLE = ("engine sh clamped to 31",)        # see coverage()


def missing(cov):
    return [k for k, v in cov.items() if (v == 0) != (k in UNREACHABLE)]


def crc(line):
    return "%08x" % zlib.crc32(line.encode())


if __name__ == "__main__":
    parent, path = sys.argv[1], sys.argv[2]
    with open(path) as f:
        lines = f.read().splitlines()
    cov = coverage(lines)
    for k, v in cov.items():
        print("%6d  %s" % (v, k))
    assert not missing(cov), missing(cov)
    crcs = [crc(l) for l in lines]
    with open(os.path.join(HERE, "requant_parent.json"), "w") as f:
        json.dump({"parent": parent, "recorded_by": "tests/golden/gen_golden_requant.py (a scratch recorder of the parent's statements)",
                   "lines": len(lines), "coverage": cov, "crc32": [" ".join(crcs[i:i + 16]) for i in range(0, len(crcs), 16)]}, f, indent=0)
        f.write("\n")
