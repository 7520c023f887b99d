// yolo355 -- one slot of y355_pipeline's ticket ring (pipeline.hip) and the device memory it takes from the pipeline's owner.
// A header of its own so that host_state_check.cpp runs the allocation on the CPU.
#pragma once
#include "y355_common.h"

struct Slot {
    float *boxes = nullptr, *scores = nullptr;      // pipeline-owned outputs of the ticket in this slot (allocated on first use)
    int32_t *cls = nullptr, *count = nullptr;
    int32_t *ovf = nullptr;                          // [max_batch] overflow flags of the ticket's forward (heads that have them)
    bool has_ovf = false;
    // what the ticket's forward wrote to (the caller's buffers or the ones above)
    float *o_boxes = nullptr, *o_scores = nullptr;
    int32_t *o_cls = nullptr, *o_count = nullptr;
    hipEvent_t done = nullptr;
    hipEvent_t released = nullptr;                   // recorded by y355_pipeline_release on the consumer's stream
    bool has_release = false;
    long long ticket = -1;
    int batch = 0;
};

// the slot's four output arrays, on first use: all of them or, after a failure (non-zero), none -- the next ticket tries again
inline int y355_slot_outputs(Slot &s, DevOwner &own, int max_batch, int max_det) {
    if (s.boxes) return 0;
    const size_t B = (size_t)max_batch, md = (size_t)max_det, mark = y355_dev_mark(own);
    Slot t = s;
    int rc = y355_dev_get(own, &t.boxes, 4 * md * B);
    rc = rc ? rc : y355_dev_get_all(own, md * B, &t.scores, &t.cls);
    rc = rc ? rc : y355_dev_get(own, &t.count, B);
    if (rc) y355_dev_rollback(own, mark);
    else s = t;
    return rc;
}
inline void y355_slot_drop_outputs(Slot &s, DevOwner &own) { y355_dev_drop(own, &s.boxes, &s.scores, &s.cls, &s.count); }
