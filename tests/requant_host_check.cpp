// The host-side derivation of the int8 fixed-point epilogue (csrc/y355_requant.h) on a fixed sweep, one line per case: the
// inputs, the return code (a refusal: its message), then every field of every struct produced and a CRC of the bias and shift
// vectors.  Asserts nothing: `make hostcheck` runs it under the address and undefined-behaviour sanitizers (no shift by a
// negative or over-wide count, no signed overflow on any input of the sweep, the refused ones included), and
// tests/test_requant_parent.py compares its lines with tests/golden/requant_parent.json, recorded from the parent commit's
// statements (tests/golden/gen_golden_requant.py).  Plain C++17: g++ -std=c++17 -Wall -Werror builds it; includes that header alone.
//
// Everything that calls the code under test is in run_engine, run_fixed, run_refresh and run_stat; the sweep and the printing
// below them know only plain numbers (the recorder replaces those four functions by the parent's statements).
#include "../yolo-compression-and-deployment-in-fpga_amd/csrc/y355_requant.h"

#include <cstdio>
#include <string>

namespace {
struct EngineCase {
    int taps, cin, sa_in, e_w, e_b, sa_out, have_out, act, retune, cout, cout_pad;
    long long wabs;                     // 0: unknown
    std::vector<int32_t> q_b;
};
struct EngineOut {
    int rc = 0;
    const char *msg = "";
    Requant rq{};
    int frac_bits = 0;
    std::vector<int32_t> bias_t;
    std::vector<long long> bias_w;
};
// one convolution of a y355_net graph.  kind: 0 a convolution, 1 the first layer (conv1.hip), 2 the first layer of a graph with
// the fused front end, 3 the second layer of such a graph, 4 a residual layer (s_r: the residual's exponent).  ew_mode: 0 one
// weight exponent for the tensor, 1 one per channel.  wabs all zero: unknown
struct NetCase {
    int kind, ksize, cin, cout, cout_pad, sa_i, e_b, lk, nm, sa_o, s_r, ew_mode;
    std::vector<int> e_wc;
    std::vector<long long> wabs;
    std::vector<int32_t> q_b;
    bool first() const { return kind == 1 || kind == 2; }
    bool front() const { return kind == 2 || kind == 3; }
    bool res() const { return kind == 4; }
};
struct FixedOut {
    int rc = 0;
    const char *msg = "";
    int F = 0, shl = 0, bshl = 0, E = 0;
    long double bmax = 0, tw = 0, tb = 0;
    std::vector<long long> bw;
    std::vector<int> shc;
};
struct RefreshOut {                      // what a forward's refresh of the layer leaves
    int rc = 0;
    const char *msg = "";
    RequantG rq{};
    ResQ rr{};                           // kind 4
    Requant rq1{};                       // kinds 1, 2
    Requant fr{};                        // kinds 2, 3
    std::vector<int32_t> bt, fb;         // the 32-bit biases uploaded for conv1.hip (kinds 1, 2) and for front.hip (kinds 2, 3)
};
struct StatOut {                         // what the statistics pass of a calibration step leaves
    int rc = 0;
    const char *msg = "";
    RequantG rq{};
    Requant rq1{};
    ResQ rr{};
    int frac_bits = 0;
};

// ---- the code under test ---------------------------------------------------------------------------------------------------
EngineOut run_engine(const EngineCase &c) {
    EngineOut o;
    Y355RqLayer q;
    const Y355RqErr e = y355_rq_layer(c.cin, c.taps, c.sa_in, c.e_w, c.e_b, c.sa_out, c.have_out != 0, c.act, c.retune, c.q_b.data(), c.cout,
                                      c.cout_pad, c.wabs, &q);
    o.rc = e.code; o.msg = e.msg;
    o.rq = q.rq; o.frac_bits = q.frac_bits; o.bias_t = q.bias_t; o.bias_w = q.bias_w;
    return o;
}
Y355RqErr fixed_of(const NetCase &c, Y355RqFixed *cf) {
    const long long K = (long long)c.ksize * c.ksize * c.cin;
    if (c.ew_mode == 0) {                // a per-tensor layer passes one exponent and its largest sum |q_w|
        const long long wmax = *std::max_element(c.wabs.begin(), c.wabs.end());
        return y355_rq_fixed(c.sa_i, &c.e_wc[0], &wmax, 1, c.e_b, c.q_b.data(), c.cout, c.cout_pad, c.lk, c.nm, K, Y355_RQ_SHL_MAX_NET, cf);
    }
    return y355_rq_fixed(c.sa_i, c.e_wc.data(), c.wabs.data(), c.cout, c.e_b, c.q_b.data(), c.cout, c.cout_pad, c.lk, c.nm, K, Y355_RQ_SHL_MAX_NET, cf);
}
FixedOut run_fixed(const NetCase &c) {
    FixedOut o;
    Y355RqFixed cf;
    const Y355RqErr e = fixed_of(c, &cf);
    o.rc = e.code; o.msg = e.msg;
    if (e.code) return o;
    o.F = cf.F; o.shl = cf.shl; o.bshl = cf.bshl; o.E = cf.E; o.bmax = cf.bmax; o.tw = cf.tw; o.tb = cf.tb; o.bw = cf.bw; o.shc = cf.shc;
    return o;
}
RefreshOut run_refresh(const NetCase &c) {
    RefreshOut o;
    Y355RqFixed cf;
    Y355RqErr e = fixed_of(c, &cf);
    if (!e.code) e = y355_rq_net(cf, c.sa_o, &o.rq);
    if (!e.code && c.res()) {
        e = y355_rq_res(cf, c.sa_o, c.s_r, &o.rr, &o.rq.narrow);
        o.rq.split = 0;
    }
    o.rc = e.code; o.msg = e.msg;
    if (e.code) return o;
    if (c.first()) {
        o.rq1 = y355_rq_first(cf, o.rq.sh);
        o.bt = o.rq1.gen32 ? y355_rq_bias32(cf) : std::vector<int32_t>(c.cout_pad, 0);
    }
    if (c.front()) {
        o.fr = y355_rq_front(cf, o.rq.sh);
        if (!o.fr.wide) o.fb = y355_rq_bias32(cf);
        o.fb.resize(c.kind == 2 ? 16 : 32, 0);
    }
    return o;
}
StatOut run_stat(const NetCase &c) {
    StatOut o;
    Y355RqFixed cf;
    Y355RqErr e = fixed_of(c, &cf);
    if (!e.code) e = y355_rq_stat(cf, c.res(), c.res() ? c.s_r : 0, &o.rq, &o.rq1, &o.rr, &o.frac_bits);
    o.rc = e.code; o.msg = e.msg;
    return o;
}

// ---- printing --------------------------------------------------------------------------------------------------------------
unsigned crc32(const void *p, size_t n) {
    unsigned c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) {
        c ^= ((const unsigned char *)p)[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
    }
    return ~c;
}
template <typename T> unsigned crc_of(const std::vector<T> &v) { return crc32(v.data(), v.size() * sizeof(T)); }
struct Line {
    std::string s;
    Line &i(long long v) { s += (s.empty() ? "" : " ") + std::to_string(v); return *this; }
    Line &t(const char *v) { s += (s.empty() ? "" : " "); s += v; return *this; }
    Line &x(unsigned v) { char b[16]; snprintf(b, sizeof b, "%08x", v); return t(b); }
    Line &f(long double v) { char b[64]; snprintf(b, sizeof b, "%La", v); return t(b); }
    template <typename T> Line &v(const std::vector<T> &a) { for (const T &e : a) i((long long)e); return *this; }
    Line &rc(int code, const char *msg) { i(code); if (code) { t("\""); s += msg; s += "\""; } return *this; }
    Line &q(const Requant &r) {
        return t("R").i(r.shl).i(r.sh).i(r.leaky).i(r.guard_log2).i(r.wide).i(r.lk).i(r.sh_l).i(r.sh_r).i(r.hm1).i(r.bw).i(r.neg_mul).i(r.gen32)
            .i(r.tmax_log2).i(r.split).i(r.negsafe).i(y355_fp32_slope_ok(r)).i(y355_fp32_exact(r)).i(y355_fp32_fold(r));
    }
    Line &g(const RequantG &r) { return t("G").i(r.shl).i(r.sh).i(r.lk).i(r.neg_mul).i(r.narrow).i(r.split); }
    Line &r(const ResQ &r) { return t("Q").i(r.t_sh).i(r.r_sh).i(r.sh).i(r.p_t).i(r.p_r).i(r.p_d).i(r.n_t).i(r.n_r).i(r.n_d); }
    void end() { puts(s.c_str()); }
};

void engine_line(const EngineCase &c) {
    const EngineOut o = run_engine(c);
    Line l;
    l.t("E").i(c.taps).i(c.cin).i(c.sa_in).i(c.e_w).i(c.e_b).i(c.sa_out).i(c.have_out).i(c.act).i(c.retune).i(c.wabs).i(c.cout).i(c.cout_pad)
        .i(c.q_b[0]).t("|").rc(o.rc, o.msg);
    if (!o.rc) l.q(o.rq).i(o.frac_bits).x(crc_of(o.bias_t)).x(crc_of(o.bias_w));
    l.end();
}
void net_line(const NetCase &c) {
    const FixedOut fx = run_fixed(c);
    Line l;
    l.t("N").i(c.kind).i(c.ksize).i(c.cin).i(c.cout).i(c.cout_pad).i(c.sa_i).i(c.e_b).i(c.lk).i(c.nm).i(c.sa_o).i(c.s_r).i(c.ew_mode).t("e").v(c.e_wc)
        .t("w").v(c.wabs).t("b").v(c.q_b).t("|").rc(fx.rc, fx.msg);
    if (!fx.rc) {
        l.i(fx.F).i(fx.shl).i(fx.bshl).i(fx.E).f(fx.bmax).f(fx.tw).f(fx.tb).x(crc_of(fx.bw)).x(crc_of(fx.shc));
        const RefreshOut rf = run_refresh(c);
        l.t("|").rc(rf.rc, rf.msg);
        if (!rf.rc) {
            l.g(rf.rq);
            if (c.res()) l.r(rf.rr);
            if (c.first()) l.q(rf.rq1).x(crc_of(rf.bt));
            if (c.front()) l.q(rf.fr).x(crc_of(rf.fb));
        }
        const StatOut st = run_stat(c);
        l.t("|").rc(st.rc, st.msg);
        if (!st.rc) l.g(st.rq).q(st.rq1).r(st.rr).i(st.frac_bits);
    }
    l.end();
}

// ---- the sweep -------------------------------------------------------------------------------------------------------------
// biases of alternating sign around mag: |q_b| * 2^bshl stays below 2^62 for every bshl the rules accept (<= 40)
std::vector<int32_t> biases(int cout, int mag) {
    std::vector<int32_t> b(cout);
    for (int c = 0; c < cout; ++c) b[c] = (c & 1 ? -1 : 1) * (mag - 13 * c);
    return b;
}
const int kBiasMag[3] = {100, 30000, 1 << 22};
struct Exps { int sa_in, e_w, e_b; };
// F = 12 / shl 0; bias exponent above: shl 2; shl 6; shl 25 (the engine's limit is 30, the nets' 24); bias far below: bshl 35;
// shl 31 and bshl 41: refused by both; bshl 8: the largest biases put |t| between 2^30 and 2^31
const Exps kExps[8] = {{5, 7, 10}, {4, 6, 12}, {7, 7, 20}, {2, 3, 30}, {20, 15, 0}, {0, 0, 31}, {0, 0, -41}, {10, 8, 10}};

void engine_sweep() {
    const int taps[3] = {1, 9, 25}, cins[4] = {3, 16, 256, 1024};
    // sh = F' - sa_out asked for: below -30 refused; 32 .. 62 (wide by the rounding add); above 62 clamped
    const int shs[15] = {-31, -30, -5, -1, 0, 1, 5, 12, 22, 31, 32, 40, 62, 63, 70};
    int n = 0;
    for (int ti = 0; ti < 3; ++ti)
        for (int act = 0; act < 3; ++act)
            for (int si = 0; si < 15; ++si)
                for (int xi = 0; xi < 8; ++xi, ++n) {
                    EngineCase c{};
                    const Exps &x = kExps[xi];
                    c.taps = taps[ti]; c.cin = cins[(n / 3) % 4]; c.sa_in = x.sa_in; c.e_w = x.e_w; c.e_b = x.e_b; c.act = act;
                    const int Fp = std::max(x.sa_in + x.e_w, x.e_b) + (act == 1 ? 3 : 0);
                    c.sa_out = Fp - shs[si];
                    c.have_out = n % 11 != 0;
                    c.retune = n % 2 ? 11 : 10;
                    c.cout = 5; c.cout_pad = 16;
                    const long long K = (long long)c.taps * c.cin;
                    c.wabs = n % 3 == 0 ? 0 : n % 3 == 1 ? 3 * K + 1 : 127 * K;        // unknown, sparse weights, every weight at 127
                    c.q_b = biases(c.cout, kBiasMag[(n / 5) % 3]);
                    engine_line(c);
                }
}
void net_sweep() {
    const int acts[3][2] = {{0, 1}, {3, 1}, {11, 205}};                   // none, 0.125, 0.1 ~ 205 / 2048
    const int geo[5][2] = {{3, 3}, {3, 16}, {1, 64}, {3, 256}, {3, 1024}};    // ksize, cin
    // sh = E - sa_out asked for: outside -20 .. 62 refused; the split form of the negative branch needs 9 .. 31
    const int shs[10] = {-21, -20, -6, 0, 8, 9, 14, 31, 32, 63};
    const int spreads[3] = {0, 2, 3};
    int n = 0;
    for (int kind = 0; kind < 5; ++kind)
        for (int ai = 0; ai < 3; ++ai)
            for (int si = 0; si < 10; ++si)
                for (int xi = 0; xi < 8; ++xi, ++n) {
                    NetCase c{};
                    const Exps &x = kExps[xi];
                    c.kind = kind; c.ksize = geo[n % 5][0]; c.cin = geo[n % 5][1]; c.cout = 4; c.cout_pad = 8;
                    c.sa_i = x.sa_in; c.e_b = x.e_b; c.lk = acts[ai][0]; c.nm = acts[ai][1];
                    c.ew_mode = n % 4 == 0 ? 0 : 1;
                    const int spread = c.ew_mode ? spreads[(n / 4) % 3] : 0;
                    for (int ch = 0; ch < c.cout; ++ch) c.e_wc.push_back(x.e_w - ch % (spread + 1));
                    const int E = std::max(x.sa_in + x.e_w, x.e_b) + c.lk;
                    c.sa_o = E - shs[si];
                    const int roff[6] = {0, -4, 3, 9, 24, 70};                    // the residual's exponent against E
                    c.s_r = kind == 4 ? E + roff[(n / 8) % 6] : 0;
                    const long long K = (long long)c.ksize * c.ksize * c.cin;
                    for (int ch = 0; ch < c.cout; ++ch)
                        c.wabs.push_back(n % 3 == 0 ? 0 : n % 3 == 1 ? 3 * K + 5 * ch : 127 * K - ch);
                    c.q_b = biases(c.cout, kBiasMag[(n / 7) % 3]);
                    net_line(c);
                }
}
}  // namespace

int main() {
    engine_sweep();
    net_sweep();
    return 0;
}
