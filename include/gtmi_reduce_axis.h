/*
 * gtmi_reduce_axis.h -- C ABI of the device-side axis reduction library
 * (gt4py_amd/storage/reduce_axis.py; storage.reduce.sum(..., axis=...) and its siblings).
 *
 * The dimensions of one strided box of one or two arrays are split into a KEPT and a REDUCED
 * group; every kept cell gets the result gtmi_reduce.h defines for its sub-box (the box with
 * every kept dimension narrowed to the cell's index). Both groups are canonical on their own
 * (storage/reduce_axis.py plan_axis makes them so): no extent-1 dimension, dimensions ordered by
 * the first source's stride, slowest first, neighbours that are contiguous in every source
 * merged -- inside a group, never across the two. Cell `c` is the C-order flat index over the
 * kept group's extents; `cells` is their product (1 for an empty group) and `n`, the summands of
 * every cell, the product of the reduced extents (1 for an empty group).
 *
 * Results are structure-of-arrays in device memory: slot `s` of cell `c` is the 8-byte word
 * result[s * cells + c], with the slot numbering of gtmi_reduce.h. A slot mask (bit `s` for slot
 * `s`) names the slots a call needs: the others are neither written nor read.
 * The reference has no device reduction; there is no reference interface this replaces.
 */
#ifndef GTMI_REDUCE_AXIS_H
#define GTMI_REDUCE_AXIS_H

#include <stdint.h>

#include "gtmi_reduce.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GTMI_REDUCE_AXIS_ABI_VERSION 1
#define GTMI_REDUCE_AXIS_MAX_PARTS 4096

/* the three traversal paths (gtmi_reduce_axis_path) */
#define GTMI_REDUCE_AXIS_SEGMENT 0 /* the reduced group ends in every source's stride-1 dimension, rows >= 32 */
#define GTMI_REDUCE_AXIS_LANE 1    /* the kept group does: a lane owns a kept cell (or a 16-B vector of them) */
#define GTMI_REDUCE_AXIS_GENERIC 2 /* everything else: one kept cell per lane, flat reduced index */

#define GTMI_REDUCE_AXIS_FOLD_SLOTS 3 /* S0, S1, S2 */

typedef struct gtmi_reduce_axis_desc {
    const void* a;                            /* device address of the first source's element (0,...,0) */
    const void* b;                            /* the second source's (products a*b), or NULL */
    int64_t k_extent[GTMI_REDUCE_MAX_DIMS];   /* the kept group: > 1 each */
    int64_t k_a_stride[GTMI_REDUCE_MAX_DIMS]; /* in elements, >= 0, non-increasing */
    int64_t k_b_stride[GTMI_REDUCE_MAX_DIMS];
    int64_t r_extent[GTMI_REDUCE_MAX_DIMS];   /* the reduced group, likewise */
    int64_t r_a_stride[GTMI_REDUCE_MAX_DIMS];
    int64_t r_b_stride[GTMI_REDUCE_MAX_DIMS];
    int32_t k_ndim;                           /* 0..GTMI_REDUCE_MAX_DIMS */
    int32_t r_ndim;                           /* 0..GTMI_REDUCE_MAX_DIMS */
    int32_t dtype;                            /* GTMI_REDUCE_F32 ... */
    int32_t reserved;
} gtmi_reduce_axis_desc;

/* Parts every cell's summands are split into when `requested` is 0: 1 when the kept cells alone
 * fill the persistent grid, else enough to fill it. A positive `requested` is returned clamped to
 * [1, GTMI_REDUCE_AXIS_MAX_PARTS]. -1 for a bad descriptor. With parts > 1 a launch needs a
 * workspace of parts * slots * cells 8-byte words (slots: GTMI_REDUCE_SCAN_SLOTS for the scan,
 * GTMI_REDUCE_AXIS_FOLD_SLOTS for the folds) and a second launch folds the parts per cell. */
int gtmi_reduce_axis_parts(const gtmi_reduce_axis_desc* desc, int requested);

/* The scan of every cell: the slots of `mask` into result[GTMI_REDUCE_SCAN_SLOTS * cells].
 * `workspace` may be NULL when parts == 1. On `stream`; nothing is synchronised. 0 on success. */
int gtmi_reduce_axis_scan(const gtmi_reduce_axis_desc* desc, uint32_t mask, void* workspace, void* result, int parts,
                          void* stream);

/* The three fold sums of every cell against its absolute maximum m[c] (device memory, `cells`
 * doubles; unused for integers) and the summand count `n` of the WHOLE reduction of a cell (both
 * may cover more than this box: a partition of the reduced axes). result[3 * cells]. */
int gtmi_reduce_axis_folds(const gtmi_reduce_axis_desc* desc, const void* m, int64_t n, void* workspace, void* result,
                           int parts, void* stream);

/* The sums from scan results (slots ABSMAX, NAN, PINF, NINF are read) and fold sums, one lane per
 * cell: out[cells], doubles or int64. */
int gtmi_reduce_axis_finish_sum(const void* scan, const void* folds, int64_t cells, int64_t n, int dtype, void* out,
                                void* stream);

/* `nrec` scan results of `cells` cells each (records[(rec * GTMI_REDUCE_SCAN_SLOTS + s) * cells + c]:
 * the parts of a domain partitioned along reduced axes) into one; the slots of `mask`. */
int gtmi_reduce_axis_combine(const void* records, int nrec, int64_t cells, int dtype, uint32_t mask, void* result,
                             void* stream);

/* The path the passes take for `desc` (GTMI_REDUCE_AXIS_*), -1 for a bad descriptor. Host-only. */
int gtmi_reduce_axis_path(const gtmi_reduce_axis_desc* desc);

const char* gtmi_reduce_axis_last_error(void);
int gtmi_reduce_axis_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* GTMI_REDUCE_AXIS_H */
