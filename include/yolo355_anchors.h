/*
 * yolo355_anchors -- C ABI of the companion library libyolo355_anchors.so: fit anchor boxes to a dataset on the GPU.
 *
 * The contract is the reference's generate_ab_kmeans.py: k-means++ (init_centroids, :50-84) and Lloyd iterations
 * (do_kmeans :87-115, anchor_box_kmeans :118-156) under the distance 1 - IoU of boxes centred at the origin (iou,
 * :27-47), all in float64 with the operations in the order written there.  R restarts run side by side; the random
 * draws are inputs (first[], u[][]), never made on the device.
 *
 * Rules taken from the reference: a box's group starts at 0 and its distance at 1; a centroid wins only with
 * distance < the best so far, so the lowest index wins ties and a box nobody beats goes to group 0; a centroid (0, 0)
 * has IoU 0 with everything; the loss is the SUM of the winning distances; an empty group becomes (0, 0); the first
 * step gives old_loss, every further step s stops the fit when |old_loss - loss| < convergence or s > max_iters,
 * otherwise old_loss = loss.  The result is the centroid set, the groups and the counts of the last step; its loss is
 * the one measured against the centroids before that step.
 *
 * Order of every sum (a function of n and Y355_ANCHORS_CHUNK alone: not of the device's size, the grid, the number of
 * restarts that run beside it, or the run):
 *   fit, score   box i belongs to chunk i / CHUNK; inside a chunk thread t (0..255) adds its boxes chunk * CHUNK +
 *                j * 256 + t for j = 0, 1, 2, 3 in that order; the 64 lanes of a wave are added as a binary tree (lane l
 *                += lane l + 32, then + 16, 8, 4, 2, 1); the four waves in order; then the chunks in order.  A box that
 *                is not in a group adds +0.0, which changes nothing.
 *   k-means++    inside a chunk thread t owns the four CONSECUTIVE boxes chunk * CHUNK + 4 t + j and adds them in
 *                order (l_j: its running sum); S_t, the running sum over the threads' totals in thread order, gives
 *                the chunk's total S_256; P_c, the running sum over the chunks' totals in chunk order, gives the
 *                total.  thresh = total * u.  The prefix of a box is P_c + (S_t + l_j); the pick is the first chunk
 *                with P_c + S_256 > thresh, in it the first thread with P_c + S_(t+1) > thresh, in it the first box
 *                with P_c + (S_t + l_j) > thresh.  Every level tests a value the level above has tested, so a pick
 *                exists exactly when the total exceeds thresh.  No pick: nothing is appended, the found centroids
 *                stay compact in the order found and the unfilled slots are (0, 0).
 * The result bits of a restart are therefore a function of (boxes, draws or init, k, max_iters, convergence) alone.
 *
 * All functions return 0 or a negative Y355_ANCHORS_E* code; y355_anchors_last_error() gives the message of the last
 * failure on the calling thread.  Arguments are checked before any HIP call.  A handle is single-threaded.  The library
 * is independent of libyolo355.so (include/yolo355.h).
 */
#ifndef YOLO355_ANCHORS_H
#define YOLO355_ANCHORS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Y355_ANCHORS_MAX_K 16
#define Y355_ANCHORS_MAX_RESTARTS 64
#define Y355_ANCHORS_MAX_BOXES (1 << 28)
#define Y355_ANCHORS_CHUNK 1024        /* boxes per partial sum: part of the result's definition */

#define Y355_ANCHORS_OK 0
#define Y355_ANCHORS_EINVAL (-1)       /* bad argument */
#define Y355_ANCHORS_EHIP (-2)         /* HIP runtime error */
#define Y355_ANCHORS_ENOTREADY (-3)    /* no boxes set / no fit made */

typedef struct y355_anchors y355_anchors;

const char *y355_anchors_last_error(void);

/* Y355_ANCHORS_CHUNK of the built library */
int y355_anchors_chunk(void);

/* A handle for up to max_boxes boxes (1..Y355_ANCHORS_MAX_BOXES), max_restarts restarts (1..64) and max_k anchors
 * (1..16) on device device_id. */
int y355_anchors_create(int32_t device_id, int64_t max_boxes, int32_t max_restarts, int32_t max_k, y355_anchors **out);
void y355_anchors_destroy(y355_anchors *h);

/* The boxes of the data set, wh[n][2] = (w, h) float64 from the host; 1 <= n <= max_boxes.  A non-finite or non-positive
 * size is Y355_ANCHORS_EINVAL before any device work.  Forgets the last fit. */
int y355_anchors_set_boxes(y355_anchors *h, const double *wh, int64_t n);

/* The same from a device pointer (float64 [n][2] on the handle's device), read on `stream`; the sizes are checked on the
 * device before anything else uses them, and after a refusal the handle holds no boxes.  Returns after `stream` has
 * finished. */
int y355_anchors_set_boxes_dev(y355_anchors *h, const void *wh_dev, int64_t n, void *stream);

/* number of boxes held (0: none) */
int64_t y355_anchors_num_boxes(const y355_anchors *h);

/* Fit k anchors (1..max_k) with `restarts` restarts (1..max_restarts), each with its own start.  Exactly one of the two
 * starts is given, the other is NULL:
 *   first[restarts], u[restarts][k - 1]   k-means++: the first centroid is box first[r] (0..n-1); draw j (0 <= u < 1)
 *                                         picks centroid j + 1.  u may be NULL when k == 1.
 *   init_index[restarts][k]               the initial centroids are the boxes of these indices (0..n-1, repeats allowed)
 * max_iters >= 1 and convergence >= 0 are the reference's iters and loss_convergence.  Runs on `stream` (a hipStream_t;
 * NULL: the null stream) and returns after it has finished. */
int y355_anchors_fit(y355_anchors *h, int32_t k, int32_t restarts, int32_t max_iters, double convergence, const int32_t *first,
                     const double *u, const int32_t *init_index, void *stream);

/* Results of the last fit, to the host; every destination may be NULL.  centroids[restarts][k][2], loss[restarts],
 * iterations[restarts] (the number of do_kmeans steps), counts[restarts][k] (the sizes of the groups of the last step),
 * init_centroids[restarts][k][2] (the start: boxes copied bit for bit), *best: the restart of the lowest loss, the
 * lowest index among equals. */
int y355_anchors_get_result(y355_anchors *h, double *centroids, double *loss, int32_t *iterations, int32_t *counts,
                            double *init_centroids, int32_t *best);

/* dst[n]: the group of every box in the last step of restart `restart` */
int y355_anchors_assignments(y355_anchors *h, int32_t restart, int32_t *dst);

/* Any anchor set on the stored boxes: anchors[k][2] (finite, >= 0; k 1..max_k) from the host.  *mean_iou: the mean over
 * the boxes of the IoU with the anchor the rules above choose (0 for a box nobody beats); counts[k]: boxes per anchor;
 * best_index (or NULL) [n]: the chosen anchor of every box.  Does not disturb the results of a fit. */
int y355_anchors_score(y355_anchors *h, const double *anchors, int32_t k, double *mean_iou, int32_t *counts, int32_t *best_index);

#ifdef __cplusplus
}
#endif
#endif
