/*
 * gtmi_relayout.h -- C ABI of the device-side storage relayout library
 * (gt4py_amd/storage/relayout.py; storage.from_array / assign / contiguous).
 *
 * One call copies one box between two strided device arrays of equal shape and element size.
 * The library moves bits and knows no dtype. The descriptor is canonical (the planner in
 * storage/relayout.py makes it so): no extent-1 dimension, neighbouring dimensions that are
 * contiguous on both sides merged, dimensions ordered by the destination's stride, slowest
 * first. The reference does this copy with CuPy's elementwise assignment
 * (storage/cartesian/interface.py:325); there is no reference interface this replaces.
 */
#ifndef GTMI_RELAYOUT_H
#define GTMI_RELAYOUT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GTMI_RELAYOUT_ABI_VERSION 1
#define GTMI_RELAYOUT_MAX_DIMS 8

/* the three copy paths (gtmi_relayout_path) */
#define GTMI_RELAYOUT_ROW 0     /* both sides have stride 1 on the last dimension */
#define GTMI_RELAYOUT_TILE 1    /* stride 1 on different dimensions: 64x64 LDS transpose */
#define GTMI_RELAYOUT_GENERIC 2 /* everything else: one element per lane, destination-fastest */

/* TILE needs at least this many elements on both stride-1 dimensions (else GENERIC) */
#define GTMI_RELAYOUT_TILE_MIN 16

typedef struct gtmi_relayout_desc {
    const void* src;                             /* device address of the source's element (0,...,0) */
    void* dst;                                   /* device address of the destination's element (0,...,0) */
    int64_t extent[GTMI_RELAYOUT_MAX_DIMS];      /* > 1 each, except a lone dimension of extent 1 */
    int64_t src_stride[GTMI_RELAYOUT_MAX_DIMS];  /* in elements, >= 0 (0 = broadcast) */
    int64_t dst_stride[GTMI_RELAYOUT_MAX_DIMS];  /* in elements, > 0, decreasing; no self-overlap */
    int32_t ndim;                                /* 1..GTMI_RELAYOUT_MAX_DIMS */
    int32_t itemsize;                            /* 1, 2, 4 or 8 bytes */
} gtmi_relayout_desc;

/* Enqueues the copy on `stream` (a hipStream_t). Returns 0 on success. */
int gtmi_relayout_copy(const gtmi_relayout_desc* desc, void* stream);

/* The path gtmi_relayout_copy takes for `desc` (GTMI_RELAYOUT_*), or -1 for a bad descriptor.
 * Host-only; never touches the device. */
int gtmi_relayout_path(const gtmi_relayout_desc* desc);

const char* gtmi_relayout_last_error(void);
int gtmi_relayout_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* GTMI_RELAYOUT_H */
