/*
 * yolo355_augment -- C ABI of the companion library libyolo355_augment.so: the pixel half of the reference's
 * SSDAugmentation (utils/augmentations.py:413-431) for a list of uint8 HWC BGR frames of mixed sizes, one launch per
 * chunk of frames, straight to a normalised fp32 [n][3][dst_h][dst_w] batch.
 *
 * The random half (every draw, the whole RandomSampleCrop search, the boxes) is the host's: yolo355/augment.py draw().
 * What it leaves for the pixels is one y355_augment_params per frame:
 *
 *   virtual image   the crop window of the expanded canvas, vh x vw pixels, after crop and before mirror and resize.  The
 *                   canvas is never materialised: virtual pixel (y, x) is source pixel (y - oy, x - ox) when that lies
 *                   inside the frame and fill[] (a BGR triple on the 0..255 scale, NOT distorted) otherwise.  With
 *                   Y355_AUG_MIRROR, x is vw - 1 - x first.
 *   photometric     on source pixels only, in the reference's fp32 order, every operation rounded on its own (no fused
 *                   multiply-add, correctly rounded division), nothing clipped anywhere:
 *                     Y355_AUG_BRIGHTNESS  p += brightness
 *                     Y355_AUG_HSV         [Y355_AUG_CONTRAST with Y355_AUG_CONTRAST_FIRST: p *= contrast]
 *                                          BGR -> HSV; Y355_AUG_SATURATION: s *= saturation; Y355_AUG_HUE: h += hue, then
 *                                          `if h > 360: h -= 360`, then `if h < 0: h += 360`; HSV -> BGR
 *                                          [Y355_AUG_CONTRAST without Y355_AUG_CONTRAST_FIRST: p *= contrast]
 *                   Without Y355_AUG_HSV the colour-space round trip and everything inside the brackets is left out (it is
 *                   not the identity); flags == 0 is the identity, which makes the call a float-resize BaseTransform.
 *   resize          cv2.resize(image, (dst_w, dst_h)) on a float32 three-channel image, INTER_LINEAR, as OpenCV 4.x's
 *                   imgproc/src/resize.cpp does it (UNPINNED, see tests/augment_ref.py):
 *                     scale = src / dst in double; f = (float)((d + 0.5) * scale - 0.5); s = floor(f); f -= s
 *                     horizontal: s < 0 -> (s, f) = (0, 0); s >= vw - 1 -> (vw - 1, 0) and the pixel is S[s] alone
 *                                 (OpenCV's xmax); otherwise S[s] * (1 - f) + S[s + 1] * f
 *                     vertical:   f is kept, the two ROW INDICES s and s + 1 are clipped to 0..vh - 1;
 *                                 D = H0 * (1 - f) + H1 * f on the horizontally blended rows
 *                     vh == dst_h and vw == dst_w: OpenCV copies the image -- so does the kernel
 *                     vh == 2 dst_h and vw == 2 dst_w: OpenCV switches to INTER_AREA's integer-scale path --
 *                                 D = (0 + (((S[2y][2x] + S[2y][2x+1]) + S[2y+1][2x]) + S[2y+1][2x+1])) * 0.25f
 *   normalise       ((D / 255) - mean[c]) / std[c] with c the image's channel (BGR order), three fp32 operations
 *   store           CHW; to_rgb != 0 stores image channel c in plane 2 - c (what data/voc0712.py:140-145 delivers)
 * The result is a function of the inputs alone; the tables are computed inside the launch from (vh, vw, dst_h, dst_w), so a
 * call keeps no state, allocates nothing and uploads nothing: the per-frame descriptors travel as kernel arguments.
 *
 * All functions return 0 or a negative Y355_AUGMENT_E* code; y355_augment_last_error() gives the message of the last
 * failure on the calling thread.  Arguments are checked before any HIP call.  The library is independent of
 * libyolo355.so (include/yolo355.h); y355_augment_frame has y355_frame's layout.
 */
#ifndef YOLO355_AUGMENT_H
#define YOLO355_AUGMENT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Y355_AUGMENT_OK 0
#define Y355_AUGMENT_EINVAL (-1)       /* bad argument */
#define Y355_AUGMENT_EHIP (-2)         /* HIP runtime error */
#define Y355_AUGMENT_ENOTREADY (-3)    /* (not returned: the library has no state) */

#define Y355_AUGMENT_MAX_SIDE 16384    /* of a frame, of a virtual image and of the output */

#define Y355_AUG_BRIGHTNESS 1
#define Y355_AUG_CONTRAST 2
#define Y355_AUG_CONTRAST_FIRST 4
#define Y355_AUG_SATURATION 8
#define Y355_AUG_HUE 16
#define Y355_AUG_MIRROR 32
#define Y355_AUG_HSV 64
#define Y355_AUG_ALL_FLAGS 127

/* one frame: device pointer to uint8 [height][width][3] (any alignment), row pitch in bytes (0 = width * 3) */
typedef struct y355_augment_frame {
    const void *data_dev;
    int32_t height, width;
    int64_t row_bytes;
} y355_augment_frame;

typedef struct y355_augment_params {
    int32_t flags;                     /* Y355_AUG_* */
    float brightness, contrast, saturation, hue;
    int32_t vh, vw;                    /* the virtual image, >= 1 */
    int32_t oy, ox;                    /* the source's origin inside it, may be negative */
    float fill[3];                     /* BGR, 0..255 scale */
} y355_augment_params;

const char *y355_augment_last_error(void);

/* sizeof(y355_augment_frame) and sizeof(y355_augment_params) of the built library (either may be NULL); returns the
 * number of frames of one launch */
int y355_augment_abi(int32_t *frame_bytes, int32_t *params_bytes);

/* Pure host validation, no HIP call: nulls; n >= 1; dst_h, dst_w 1..Y355_AUGMENT_MAX_SIDE; per frame a pointer, sizes
 * 1..Y355_AUGMENT_MAX_SIDE, row_bytes 0 or >= 3 * width; vh, vw 1..Y355_AUGMENT_MAX_SIDE; |oy|, |ox| <= 2^24; known flags;
 * finite brightness / contrast / saturation / hue / fill; finite mean, finite non-zero std. */
int y355_augment_check(const y355_augment_frame *frames, const y355_augment_params *params, int32_t n, int32_t dst_h, int32_t dst_w,
                       const float *mean, const float *std);

/* The checks above and device_id >= 0, dst_dev != NULL; then the launches on `stream` (a hipStream_t of device device_id;
 * NULL: the null stream) that write float32 dst_dev[n][3][dst_h][dst_w].  Asynchronous: returns once everything is enqueued;
 * the frames must stay valid until the stream has run it.  The caller's current device is left as it was. */
int y355_augment_run(int32_t device_id, const y355_augment_frame *frames, const y355_augment_params *params, int32_t n, int32_t dst_h,
                     int32_t dst_w, const float *mean, const float *std, int32_t to_rgb, void *dst_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif
