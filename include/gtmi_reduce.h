/*
 * gtmi_reduce.h -- C ABI of the device-side domain reduction library
 * (gt4py_amd/storage/reduce.py; storage.reduce.sum / dot / min / max / absmax / ...).
 *
 * A reduction runs over one strided box of one array, or over the element-wise products of the
 * same box of two arrays. The descriptor is canonical (storage/reduce.py makes it so): no
 * extent-1 dimension, neighbouring dimensions that are contiguous in both sources merged,
 * dimensions ordered by the first source's stride, slowest first. The summands are f64 for
 * f32 / f64 sources (a product is one f64 multiply) and int64 with wrap-around for int32 /
 * int64 sources. Every result is a function of the multiset of summands only, not of the grid
 * or of the traversal order: the numpy restatement in storage/reduce.py is the definition.
 * The reference has no device reduction; there is no reference interface this replaces.
 */
#ifndef GTMI_REDUCE_H
#define GTMI_REDUCE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GTMI_REDUCE_ABI_VERSION 1
#define GTMI_REDUCE_MAX_DIMS 8
#define GTMI_REDUCE_MAX_BLOCKS 65536

/* element types of the sources */
#define GTMI_REDUCE_F32 0
#define GTMI_REDUCE_F64 1
#define GTMI_REDUCE_I32 2
#define GTMI_REDUCE_I64 3

/* the two traversal paths (gtmi_reduce_path) */
#define GTMI_REDUCE_ROW 0     /* every source has stride 1 on the last dimension, rows of >= 32 elements */
#define GTMI_REDUCE_GENERIC 1 /* everything else: one element per lane of the flat index */

/* The scan result: GTMI_REDUCE_SCAN_SLOTS 8-byte slots, doubles for f32 / f64 sources and
 * int64 for int32 / int64 sources where marked (V). NaN summands are counted and otherwise
 * left out of slots 0..2 (identities: absmax 0, min +inf / INT64_MAX, max -inf / INT64_MIN);
 * -0.0 orders below +0.0. Slots 8..10 repeat 0..2 with numpy's NaN propagation. */
#define GTMI_REDUCE_SCAN_ABSMAX 0     /* (V) */
#define GTMI_REDUCE_SCAN_MIN 1        /* (V) */
#define GTMI_REDUCE_SCAN_MAX 2        /* (V) */
#define GTMI_REDUCE_SCAN_NAN 3        /* int64 */
#define GTMI_REDUCE_SCAN_PINF 4       /* int64 */
#define GTMI_REDUCE_SCAN_NINF 5       /* int64 */
#define GTMI_REDUCE_SCAN_NONFINITE 6  /* int64: the three counts added */
#define GTMI_REDUCE_SCAN_ABSMAX_NAN 8 /* (V): NaN when any summand is */
#define GTMI_REDUCE_SCAN_MIN_NAN 9    /* (V) */
#define GTMI_REDUCE_SCAN_MAX_NAN 10   /* (V) */
#define GTMI_REDUCE_SCAN_SLOTS 12
#define GTMI_REDUCE_FOLD_SLOTS 4 /* S0, S1, S2 (V), one spare */

typedef struct gtmi_reduce_desc {
    const void* a;                            /* device address of the first source's element (0,...,0) */
    const void* b;                            /* the second source's (products a*b), or NULL */
    int64_t extent[GTMI_REDUCE_MAX_DIMS];     /* > 1 each, except a lone dimension of extent 1 */
    int64_t a_stride[GTMI_REDUCE_MAX_DIMS];   /* in elements, >= 0, non-increasing */
    int64_t b_stride[GTMI_REDUCE_MAX_DIMS];   /* in elements, >= 0 (ignored without b) */
    int32_t ndim;                             /* 1..GTMI_REDUCE_MAX_DIMS */
    int32_t dtype;                            /* GTMI_REDUCE_F32 ... */
} gtmi_reduce_desc;

/* Blocks a launch over `desc` uses when `requested` is 0: a persistent grid sized from the
 * current device's CU count, fewer for a box with less work than that. A positive `requested`
 * is returned clamped to [1, GTMI_REDUCE_MAX_BLOCKS]. -1 for a bad descriptor. The workspace of
 * a launch holds that many records of GTMI_REDUCE_SCAN_SLOTS (scan) or GTMI_REDUCE_FOLD_SLOTS
 * (folds) 8-byte slots. */
int gtmi_reduce_blocks(const gtmi_reduce_desc* desc, int requested);

/* One pass over the box: `blocks` partial records into `workspace`, then a one-block launch that
 * folds them into `result` (GTMI_REDUCE_SCAN_SLOTS slots, device memory). Both on `stream`
 * (a hipStream_t); nothing is synchronised. Returns 0 on success. */
int gtmi_reduce_scan(const gtmi_reduce_desc* desc, void* workspace, void* result, int blocks, void* stream);

/* One pass over the box: the three fold sums of the summands, pre-rounded against the absolute
 * maximum `*m` (device memory: a double for f32 / f64 sources, unused for integers) and the
 * summand count `n` of the WHOLE reduction (both may cover more than this box: a partition of a
 * larger domain). `result` gets GTMI_REDUCE_FOLD_SLOTS slots. Non-finite summands count as 0. */
int gtmi_reduce_folds(const gtmi_reduce_desc* desc, const void* m, int64_t n, void* workspace, void* result,
                      int blocks, void* stream);

/* The sum from a scan result and fold sums (device memory both): the non-finite rules, +0.0 for
 * an absolute maximum of 0, else S0 + (S1 + S2) scaled back; one 8-byte slot into `out`. */
int gtmi_reduce_finish_sum(const void* scan, const void* folds, int64_t n, int dtype, void* out, void* stream);

/* `nrec` scan results (GTMI_REDUCE_SCAN_SLOTS slots each, contiguous in device memory: the
 * parts of a partitioned domain) into one, by the rules of the scan itself. */
int gtmi_reduce_combine(const void* records, int nrec, int dtype, void* result, void* stream);

/* The path the two passes take for `desc` (GTMI_REDUCE_*), -1 for a bad descriptor. Host-only. */
int gtmi_reduce_path(const gtmi_reduce_desc* desc);

const char* gtmi_reduce_last_error(void);
int gtmi_reduce_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* GTMI_REDUCE_H */
