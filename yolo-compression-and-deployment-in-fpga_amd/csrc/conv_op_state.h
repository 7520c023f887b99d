// yolo355 -- the device memory of a y355_conv_op (ops.hip): every pointer of the operator, and the keys that say what the memory
// holds now -- which packed weights, and the geometry each workspace was last zeroed for.  Nothing of a kernel launcher: a header
// of its own so that host_state_check.cpp runs the allocation logic on the CPU.
#pragma once
#include "y355_common.h"

struct ConvOpMem {
    DevOwner own;
    // the packed weights for kernel w_kid at w_cout_pad output channels, with the bias vector that is padded alike: fp32
    // (bias_dev) for a bf16 operator, 64-bit (bw_dev, filled per input exponent) for an int8 one; w_kid -1: nothing packed
    char *w_dev = nullptr;
    float *bias_dev = nullptr;
    long long *bw_dev = nullptr;
    int w_kid = -1, w_cout_pad = 0;
    // int8, from the create: [0] absmax bits, [1] non-dyadic count; 3x3 only: the 32-bit biases and the counters
    unsigned int *flag_dev = nullptr;
    int *bt_dev = nullptr;
    Counters *ctr_dev = nullptr;
    // workspaces (grown on demand), and the geometry word (never 0) each was last zeroed for on the caller's stream.  The
    // staging kernels write the interior and the real channels only, so the halo and the padding channels stay zero for as
    // long as the geometry does.
    char *in_dev = nullptr, *out_dev = nullptr, *res_dev = nullptr;
    size_t in_cap = 0, out_cap = 0, res_cap = 0;
    size_t in_geo = 0, out_geo = 0, res_geo = 0;
};
struct ConvOpZero {                    // the workspaces a forward has to zero on its stream before it stages
    bool in = false, out = false, res = false;
};

// the create-time buffers of an int8 operator (cout_pad 0: general geometry, the flag words alone): all of them or, after a
// failure, none
inline int y355_convop_create_i8(ConvOpMem &m, int cout_pad) {
    int rc = y355_dev_get(m.own, &m.flag_dev, 4);
    if (cout_pad) {
        rc = rc ? rc : y355_dev_get(m.own, &m.bt_dev, (size_t)cout_pad);
        rc = rc ? rc : y355_dev_get(m.own, &m.ctr_dev, 1);
    }
    if (rc) y355_dev_drop(m.own, &m.flag_dev, &m.bt_dev, &m.ctr_dev);
    return rc;
}

// The weights for another (kernel id, padded width): `packed`, and bias_f (cout_pad floats) or, null, room for an int8
// operator's 64-bit biases.  The new buffers are taken first and the old ones dropped after, so a failure leaves the old
// fragments AND the old key: the key never names fragments that are gone.  Nothing on `s` may still read the old ones.
inline int y355_convop_swap_weights(ConvOpMem &m, int kid, int cout_pad, const std::vector<char> &packed, const float *bias_f, hipStream_t s) {
    const size_t mark = y355_dev_mark(m.own);
    char *w = nullptr;
    float *bf = nullptr;
    long long *bw = nullptr;
    int rc = y355_dev_get(m.own, &w, packed.size());
    rc = rc ? rc : m.own.mem.upload(w, packed.data(), packed.size(), s);
    if (bias_f) {
        rc = rc ? rc : y355_dev_get(m.own, &bf, (size_t)cout_pad);
        rc = rc ? rc : m.own.mem.upload(bf, bias_f, sizeof(float) * cout_pad, s);
    } else {
        rc = rc ? rc : y355_dev_get(m.own, &bw, (size_t)cout_pad);
    }
    if (rc) {
        y355_dev_rollback(m.own, mark);
        return rc;
    }
    y355_dev_drop(m.own, &m.w_dev, &m.bias_dev, &m.bw_dev);
    m.w_dev = w, m.bias_dev = bf, m.bw_dev = bw;
    m.w_kid = kid, m.w_cout_pad = cout_pad;
    m.out_geo = m.res_geo = 0;         // their layouts depend on the padded width
    return 0;
}

// one workspace at `bytes`: new memory comes zeroed, but on no stream in particular, so it counts as zeroed for no geometry
inline int y355_convop_grow(ConvOpMem &m, char **p, size_t *cap, size_t *zeroed_for, size_t bytes) {
    if (bytes > *cap || !*p) *zeroed_for = 0;
    return y355_dev_grow<true>(m.own, cap, bytes, p);
}
// The workspaces of one forward at geometry `geo`: in, out and (res_bytes != 0) the residual's, grown where too small.  *z: what
// the caller zeroes on its stream -- every buffer last zeroed for another geometry; out only where out_halo says that its
// halo is read (a property of the operator: the int8 results and the general geometry's outputs are written whole).  Once
// that is enqueued the caller says so with y355_convop_zeroed; until then, and after a failure, the recorded geometries stand.
inline int y355_convop_workspaces(ConvOpMem &m, size_t geo, size_t in_bytes, size_t out_bytes, bool out_halo, size_t res_bytes, ConvOpZero *z) {
    int rc = y355_convop_grow(m, &m.in_dev, &m.in_cap, &m.in_geo, in_bytes);
    rc = rc ? rc : y355_convop_grow(m, &m.out_dev, &m.out_cap, &m.out_geo, out_bytes);
    if (res_bytes) rc = rc ? rc : y355_convop_grow(m, &m.res_dev, &m.res_cap, &m.res_geo, res_bytes);
    if (rc) return rc;
    z->in = m.in_geo != geo;
    z->out = out_halo && m.out_geo != geo;
    z->res = res_bytes && m.res_geo != geo;
    return 0;
}
inline void y355_convop_zeroed(ConvOpMem &m, size_t geo, const ConvOpZero &z) {
    if (z.in) m.in_geo = geo;
    if (z.out) m.out_geo = geo;
    if (z.res) m.res_geo = geo;
}

// everything goes back; idempotent
inline void y355_convop_close(ConvOpMem &m) {
    y355_dev_release_all(m.own);
    const DevMem mem = m.own.mem;
    m = ConvOpMem{};
    m.own.mem = mem;
}
