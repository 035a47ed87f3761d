// gtmi_reduce_axis.hip -- reductions over some dimensions of one strided box of one or two device
// arrays, one result per cell of the others (storage.reduce.*(axis=...);
// include/gtmi_reduce_axis.h). The numpy restatement in storage/reduce_axis.py defines every
// result: cell c gets what gtmi_reduce.hip gives for the sub-box of c. The per-summand rules are
// those of gtmi_reduce.hip, shared through gtmi_reduce_rules.h; the fold plan is per cell, from
// the cell's own absolute maximum m[c] and the count n every cell shares.
//
// Passes as in gtmi_reduce.hip (scan; folds against m[] and n; finish; combine of partitions),
// results structure-of-arrays: slot s of cell c at result[s * cells + c]. Three traversal paths,
// chosen on the host from the canonical descriptor (kept group, reduced group):
//   SEGMENT  the reduced group ends in every source's stride-1 dimension (rows of at least
//            GTMI_REDUCE_SHORT_ROW): the row machinery of gtmi_reduce_rows per kept cell. A work
//            item is (cell, part) and belongs to one wave: it walks units part, part + parts, ...
//            of the cell's (row, 64-lane chunk) units, 16 B per lane when every row of every
//            source shares its 16-B phase, element-wise heads and tails; outer indices and the
//            cell are wave-uniform. The wave folds its lanes with gtmi::shfl and lane 0 stores;
//   LANE     the kept group ends in the stride-1 dimension (rows of at least 32 cells): a lane
//            owns one kept cell, or a 16-B vector of them, and marches over a contiguous range of
//            the flat reduced index with wave-uniform offsets, GTMI_AXIS_UNROLL loads in flight;
//            no cross-lane step. A work item is (kept row, 64-lane chunk, part), one wave each;
//   GENERIC  everything else: one (cell, part) per lane, both indices decomposed per element.
// With parts == 1 the traversal writes the finished slots; else it writes part records
// ws[(part * slots + s) * cells + c] and a second launch, one lane per cell, folds them.
// No atomics, no LDS, no inter-block protocol, no host synchronisation. All offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "gtmi_device.h"
#include "gtmi_roctx.h"

#include "gtmi_reduce_axis.h"
#include "gtmi_reduce_rules.h"  // summands, scan update, fold plan, fold step, finish

#define GTMI_AXIS_UNROLL 4         // loads in flight per lane and trip
#define GTMI_AXIS_BLOCKS_PER_CU 8  // persistent grid: 32 waves per CU
#define GTMI_AXIS_THREADS 256
#define GTMI_AXIS_WAVES (GTMI_AXIS_THREADS / 64)
#define GTMI_AXIS_LANE_WAVES_PER_CU 16  // gtmi_axis_lane: up to 122 VGPRs, 4 waves per SIMD

static thread_local char g_err[512];

struct AxBox {  // the descriptor as the kernels take it (by value)
    const char* a;
    const char* b;
    int64_t kext[GTMI_REDUCE_MAX_DIMS], kas[GTMI_REDUCE_MAX_DIMS], kbs[GTMI_REDUCE_MAX_DIMS];
    int64_t rext[GTMI_REDUCE_MAX_DIMS], ras[GTMI_REDUCE_MAX_DIMS], rbs[GTMI_REDUCE_MAX_DIMS];
    int64_t cells, nred;  // products of the kept / reduced extents
    int32_t nk, nr;
};

struct Pass {  // what every traversal kernel takes besides the box
    const double* m;  // per-cell absolute maxima (float folds), else unused
    uint64_t* out;    // the result (final) or the part records
    int32_t L, parts, final, head;
    uint32_t mask;
};

// ------------------------------------------------------------------ records in SoA form
// base slots (0..5) a mask of result slots is computed from
static uint32_t base_mask(uint32_t mask) {
    uint32_t b = mask & 0x3fu;
    if (mask & (1u << GTMI_REDUCE_SCAN_NONFINITE)) b |= 0x38u;
    if (mask & (1u << GTMI_REDUCE_SCAN_ABSMAX_NAN)) b |= 0x09u;
    if (mask & (1u << GTMI_REDUCE_SCAN_MIN_NAN)) b |= 0x0au;
    if (mask & (1u << GTMI_REDUCE_SCAN_MAX_NAN)) b |= 0x0cu;
    return b;
}

template <typename Acc> struct AccIO;

template <typename V> struct AccIO<ScanAcc<V>> {
    static constexpr int SLOTS = GTMI_REDUCE_SCAN_SLOTS;
    // final: the finished slots of `mask`; else: the base slots of `mask` (a part record)
    static GTMI_DEV void store(const ScanAcc<V>& acc, uint64_t* p, int64_t cells, uint32_t mask, bool final) {
        uint64_t r[GTMI_REDUCE_SCAN_SLOTS];
        acc.finish(r);
        const int n = final ? GTMI_REDUCE_SCAN_SLOTS : 6;
#pragma unroll
        for (int s = 0; s < GTMI_REDUCE_SCAN_SLOTS; ++s)
            if (s < n && ((mask >> s) & 1u)) p[(int64_t)s * cells] = r[s];
    }
    static GTMI_DEV void load(ScanAcc<V>& acc, const uint64_t* p, int64_t cells, uint32_t bmask) {
        acc.init();
        if (bmask & 1u) acc.absmax = value_of<V>(p[0]);
        if (bmask & 2u) acc.mn = value_of<V>(p[cells]);
        if (bmask & 4u) acc.mx = value_of<V>(p[2 * cells]);
        if (bmask & 8u) acc.nan = (int64_t)p[3 * cells];
        if (bmask & 16u) acc.pinf = (int64_t)p[4 * cells];
        if (bmask & 32u) acc.ninf = (int64_t)p[5 * cells];
    }
};

template <> struct AccIO<FoldAcc<double>> {
    static constexpr int SLOTS = GTMI_REDUCE_AXIS_FOLD_SLOTS;
    static GTMI_DEV void store(const FoldAcc<double>& acc, uint64_t* p, int64_t cells, uint32_t, bool) {
        p[0] = bits_of(acc.s0);
        p[cells] = bits_of(acc.s1);
        p[2 * cells] = bits_of(acc.s2);
    }
    static GTMI_DEV void load(FoldAcc<double>& acc, const uint64_t* p, int64_t cells, uint32_t) {
        acc.s0 = double_of(p[0]);
        acc.s1 = double_of(p[cells]);
        acc.s2 = double_of(p[2 * cells]);
    }
};

template <> struct AccIO<FoldAcc<int64_t>> {
    static constexpr int SLOTS = GTMI_REDUCE_AXIS_FOLD_SLOTS;
    static GTMI_DEV void store(const FoldAcc<int64_t>& acc, uint64_t* p, int64_t cells, uint32_t, bool) {
        p[0] = acc.s0;
        p[cells] = 0;
        p[2 * cells] = 0;
    }
    static GTMI_DEV void load(FoldAcc<int64_t>& acc, const uint64_t* p, int64_t, uint32_t) { acc.s0 = p[0]; }
};

// where item (cell, part) of a pass stores
template <typename Acc> GTMI_DEV uint64_t* record_of(const Pass& ps, int64_t cells, int64_t cell, int64_t part) {
    return ps.out + (ps.final ? cell : (part * AccIO<Acc>::SLOTS) * cells + cell);
}

// the per-summand constants of a cell: its fold plan from (m[cell], L) for the float folds
template <typename Acc> GTMI_DEV typename Acc::Params cell_params(const Pass& ps, int64_t cell) {
    if constexpr (std::is_same<Acc, FoldAcc<double>>::value)
        return typename Acc::Params(ps.m[cell], ps.L);
    else
        return typename Acc::Params(0.0, ps.L);
}

// ------------------------------------------------------------------ index decomposition
// Offsets of flat index `c` over the first `nd` kept dimensions.
GTMI_DEV void kept_offsets(const AxBox& bx, int64_t c, int nd, int64_t& oa, int64_t& ob) {
    oa = 0;
    ob = 0;
    for (int d = nd - 1; d >= 0; --d) {
        const int64_t e = bx.kext[d], q = c / e, idx = c - q * e;
        oa += idx * bx.kas[d];
        ob += idx * bx.kbs[d];
        c = q;
    }
}
// Offsets of flat index `r` over the first `nd` reduced dimensions.
GTMI_DEV void red_offsets(const AxBox& bx, int64_t r, int nd, int64_t& oa, int64_t& ob) {
    oa = 0;
    ob = 0;
    for (int d = nd - 1; d >= 0; --d) {
        const int64_t e = bx.rext[d], q = r / e, idx = r - q * e;
        oa += idx * bx.ras[d];
        ob += idx * bx.rbs[d];
        r = q;
    }
}

// ------------------------------------------------------------------ kernels
// SEGMENT. VEC elements per lane and access: 16 / sizeof(T) when every row of every source starts
// `head` elements past a 16-B line, else 1 with head 0 (gtmi_reduce_rows, per kept cell).
template <typename T, int VEC, bool TWO, typename Acc>
__global__ void __launch_bounds__(GTMI_AXIS_THREADS) gtmi_axis_segment(const AxBox bx, const Pass ps) {
    using Vt = gtmi::evec<T, VEC>;
    constexpr int U = GTMI_AXIS_UNROLL;
    const int lane = (int)(threadIdx.x & 63);
    const int head = ps.head;
    const int last = bx.nr - 1;
    const int64_t n = bx.rext[last];
    const int64_t nvec = (head + n + VEC - 1) / VEC;
    const int64_t cpr = (nvec + 64 * U - 1) / (64 * U);
    const int64_t units = (bx.nred / n) * cpr;
    const int64_t parts = ps.parts;
    const int64_t items = bx.cells * parts;
    const int64_t nwaves = (int64_t)gridDim.x * GTMI_AXIS_WAVES;
    const int64_t w0 = (int64_t)blockIdx.x * GTMI_AXIS_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const T* __restrict__ a = (const T*)bx.a;
    const T* __restrict__ b = (const T*)bx.b;
    for (int64_t item = w0; item < items; item += nwaves) {
        const int64_t cell = item / parts, part = item - cell * parts;
        int64_t ca, cb;
        kept_offsets(bx, cell, bx.nk, ca, cb);
        const typename Acc::Params prm = cell_params<Acc>(ps, cell);
        Acc acc;
        acc.init();
        for (int64_t u = part; u < units; u += parts) {
            const int64_t row = u / cpr, c = u - row * cpr;
            int64_t oa, ob;
            red_offsets(bx, row, last, oa, ob);
            const T* __restrict__ ra = a + ca + oa;
            const T* __restrict__ rb = TWO ? b + cb + ob : nullptr;
            int64_t e0[U];
            bool whole[U];
            Vt va[U], vb[U];
#pragma unroll
            for (int k = 0; k < U; ++k) {  // the whole vectors of the trip first: all loads in flight together
                e0[k] = ((c * U + k) * 64 + lane) * VEC - head;
                whole[k] = e0[k] >= 0 && e0[k] + VEC <= n;
                va[k] = Vt{};
                vb[k] = Vt{};
                if (whole[k]) {
                    va[k] = *(const Vt*)(ra + e0[k]);
                    if constexpr (TWO) vb[k] = *(const Vt*)(rb + e0[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < U; ++k) {
                if (whole[k]) {
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        if constexpr (TWO)
                            acc.add(product(summand(va[k][j]), summand(vb[k][j])), prm);
                        else
                            acc.add(summand(va[k][j]), prm);
                    }
                } else if constexpr (VEC > 1) {  // a vector that sticks out of the row: its elements inside [0, n)
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        const int64_t e = e0[k] + j;
                        if (e >= 0 && e < n) {
                            if constexpr (TWO)
                                acc.add(product(summand(ra[e]), summand(rb[e])), prm);
                            else
                                acc.add(summand(ra[e]), prm);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int delta = 32; delta >= 1; delta >>= 1) {  // every lane of the wave is here: item is wave-uniform
            const Acc o = acc.shuffled(delta);
            acc.combine(o);
        }
        if (lane == 0) AccIO<Acc>::store(acc, record_of<Acc>(ps, bx.cells, cell, part), bx.cells, ps.mask, ps.final != 0);
    }
}

// LANE. A lane owns the VEC kept cells e0 .. e0 + VEC - 1 of a kept row (those inside the row) and
// marches over the reduced indices [r0, r1) of its part. The offsets of a reduced index are
// wave-uniform: the innermost reduced dimension steps by its stride, the outer ones are decomposed
// again when it wraps.
template <typename T, int VEC, bool TWO, typename Acc>
__global__ void __launch_bounds__(GTMI_AXIS_THREADS) gtmi_axis_lane(const AxBox bx, const Pass ps) {
    using Vt = gtmi::evec<T, VEC>;
    constexpr int U = GTMI_AXIS_UNROLL;
    const int lane = (int)(threadIdx.x & 63);
    const int head = ps.head;
    const int klast = bx.nk - 1;
    const int64_t nrow = bx.kext[klast];
    const int64_t nvec = (head + nrow + VEC - 1) / VEC;
    const int64_t cpr = (nvec + 63) / 64;
    const int64_t krows = bx.cells / nrow;
    const int64_t parts = ps.parts;
    const int64_t per = (bx.nred + parts - 1) / parts;
    const int64_t items = krows * cpr * parts;
    const int64_t nwaves = (int64_t)gridDim.x * GTMI_AXIS_WAVES;
    const int64_t w0 = (int64_t)blockIdx.x * GTMI_AXIS_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int rlast = bx.nr - 1;
    const int64_t ni = bx.nr > 0 ? bx.rext[rlast] : 1;
    const int64_t ia = bx.nr > 0 ? bx.ras[rlast] : 0, ib = bx.nr > 0 ? bx.rbs[rlast] : 0;
    const T* __restrict__ a = (const T*)bx.a;
    const T* __restrict__ b = (const T*)bx.b;
    for (int64_t item = w0; item < items; item += nwaves) {
        const int64_t t = item / parts, part = item - t * parts;
        const int64_t krow = t / cpr, ch = t - krow * cpr;
        int64_t ca, cb;
        kept_offsets(bx, krow, klast, ca, cb);
        const int64_t e0 = (ch * 64 + lane) * VEC - head;
        const bool whole = e0 >= 0 && e0 + VEC <= nrow;
        const int64_t cell0 = krow * nrow + e0;
        bool valid[VEC];
        typename Acc::Params prm[VEC];
        Acc acc[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            valid[j] = e0 + j >= 0 && e0 + j < nrow;
            if (valid[j]) prm[j] = cell_params<Acc>(ps, cell0 + j);
            acc[j].init();
        }
        const T* __restrict__ la = a + ca + e0;
        const T* __restrict__ lb = TWO ? b + cb + e0 : nullptr;
        const int64_t r0 = part * per, r1 = r0 + per < bx.nred ? r0 + per : bx.nred;
        int64_t o = r0 / ni, i = r0 - o * ni, oa, ob;
        red_offsets(bx, o, rlast, oa, ob);
        int64_t pa = oa + i * ia, pb = ob + i * ib;
        for (int64_t r = r0; r < r1; r += U) {
            const int64_t cnt = r1 - r;  // reduced indices of this trip: min(U, cnt)
            int64_t offa[U], offb[U];
#pragma unroll
            for (int k = 0; k < U; ++k) {
                offa[k] = pa;
                offb[k] = pb;
                if (++i == ni) {  // the innermost reduced dimension wraps (offsets past r1 are never used)
                    i = 0;
                    ++o;
                    red_offsets(bx, o, rlast, oa, ob);
                    pa = oa;
                    pb = ob;
                } else {
                    pa += ia;
                    pb += ib;
                }
            }
            Vt va[U], vb[U];
#pragma unroll
            for (int k = 0; k < U; ++k) {  // all loads of the trip in flight together
                va[k] = Vt{};
                vb[k] = Vt{};
                if (k < cnt) {
                    if (whole) {
                        va[k] = *(const Vt*)(la + offa[k]);
                        if constexpr (TWO) vb[k] = *(const Vt*)(lb + offb[k]);
                    } else if constexpr (VEC > 1) {  // a vector that sticks out of the kept row
#pragma unroll
                        for (int j = 0; j < VEC; ++j) {
                            if (valid[j]) {
                                va[k][j] = la[offa[k] + j];
                                if constexpr (TWO) vb[k][j] = lb[offb[k] + j];
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < U; ++k) {
                if (k < cnt) {
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        if (valid[j]) {
                            if constexpr (TWO)
                                acc[j].add(product(summand(va[k][j]), summand(vb[k][j])), prm[j]);
                            else
                                acc[j].add(summand(va[k][j]), prm[j]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j)
            if (valid[j])
                AccIO<Acc>::store(acc[j], record_of<Acc>(ps, bx.cells, cell0 + j, part), bx.cells, ps.mask, ps.final != 0);
    }
}

// GENERIC: one (cell, part) per lane, any strides (0 included).
template <typename T, bool TWO, typename Acc>
__global__ void __launch_bounds__(GTMI_AXIS_THREADS) gtmi_axis_flat(const AxBox bx, const Pass ps) {
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    const int64_t parts = ps.parts;
    const int64_t per = (bx.nred + parts - 1) / parts;
    const int64_t items = bx.cells * parts;
    const T* __restrict__ a = (const T*)bx.a;
    const T* __restrict__ b = (const T*)bx.b;
    for (int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; item < items; item += nthreads) {
        const int64_t part = item / bx.cells, cell = item - part * bx.cells;
        int64_t ca, cb;
        kept_offsets(bx, cell, bx.nk, ca, cb);
        const typename Acc::Params prm = cell_params<Acc>(ps, cell);
        Acc acc;
        acc.init();
        const int64_t r0 = part * per, r1 = r0 + per < bx.nred ? r0 + per : bx.nred;
        for (int64_t r = r0; r < r1; ++r) {
            int64_t oa, ob;
            red_offsets(bx, r, bx.nr, oa, ob);
            if constexpr (TWO)
                acc.add(product(summand(a[ca + oa]), summand(b[cb + ob])), prm);
            else
                acc.add(summand(a[ca + oa]), prm);
        }
        AccIO<Acc>::store(acc, record_of<Acc>(ps, bx.cells, cell, part), bx.cells, ps.mask, ps.final != 0);
    }
}

// `nrec` records per cell (recs[(rec * SLOTS + s) * cells + c]) into the result, one lane per cell.
template <typename Acc>
__global__ void __launch_bounds__(GTMI_AXIS_THREADS) gtmi_axis_records(const uint64_t* __restrict__ recs, int nrec, int64_t cells,
                                                                     uint32_t mask, uint32_t bmask,
                                                                     uint64_t* __restrict__ result) {
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += nthreads) {
        Acc acc;
        acc.init();
        for (int64_t i = 0; i < nrec; ++i) {
            Acc o;
            AccIO<Acc>::load(o, recs + (i * AccIO<Acc>::SLOTS) * cells + c, cells, bmask);
            acc.combine(o);
        }
        AccIO<Acc>::store(acc, result + c, cells, mask, true);
    }
}

__global__ void __launch_bounds__(GTMI_AXIS_THREADS) gtmi_axis_finish(const uint64_t* __restrict__ scan,
                                                                    const uint64_t* __restrict__ folds, int64_t cells, int L,
                                                                    int floating, uint64_t* __restrict__ out) {
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += nthreads) {
        if (!floating) {
            out[c] = folds[c];
            continue;
        }
        const int64_t nan = (int64_t)scan[GTMI_REDUCE_SCAN_NAN * cells + c];
        const int64_t pinf = (int64_t)scan[GTMI_REDUCE_SCAN_PINF * cells + c];
        const int64_t ninf = (int64_t)scan[GTMI_REDUCE_SCAN_NINF * cells + c];
        const double M = double_of(scan[GTMI_REDUCE_SCAN_ABSMAX * cells + c]);
        out[c] = bits_of(finish_sum(nan, pinf, ninf, M, double_of(folds[c]), double_of(folds[cells + c]),
                                    double_of(folds[2 * cells + c]), L));
    }
}

// ------------------------------------------------------------------ host side
extern "C" const char* gtmi_reduce_axis_last_error(void) { return g_err; }
extern "C" int gtmi_reduce_axis_abi_version(void) { return GTMI_REDUCE_AXIS_ABI_VERSION; }

static int itemsize_of(int dtype) { return (dtype == GTMI_REDUCE_F32 || dtype == GTMI_REDUCE_I32) ? 4 : 8; }

static int64_t product_of(const int64_t* ext, int nd) {
    int64_t p = 1;
    for (int i = 0; i < nd; ++i) p *= ext[i];
    return p;
}

static bool group_ok(const char* name, const int64_t* ext, const int64_t* as, const int64_t* bs, int nd, bool two) {
    if (nd < 0 || nd > GTMI_REDUCE_MAX_DIMS) {
        snprintf(g_err, sizeof(g_err), "bad descriptor: %s ndim=%d", name, nd);
        return false;
    }
    for (int i = 0; i < nd; ++i) {
        if (ext[i] < 1 || as[i] < 0 || (two && bs[i] < 0)) {
            snprintf(g_err, sizeof(g_err), "%s dimension %d: extent=%lld a_stride=%lld b_stride=%lld", name, i,
                     (long long)ext[i], (long long)as[i], (long long)bs[i]);
            return false;
        }
    }
    return true;
}

// Validates `d`; returns the path, -1 on error (g_err set).
static int choose_path(const gtmi_reduce_axis_desc* d) {
    g_err[0] = 0;
    if (d == NULL) {
        snprintf(g_err, sizeof(g_err), "null descriptor");
        return -1;
    }
    if (d->dtype < GTMI_REDUCE_F32 || d->dtype > GTMI_REDUCE_I64) {
        snprintf(g_err, sizeof(g_err), "bad descriptor: dtype=%d", (int)d->dtype);
        return -1;
    }
    const bool two = d->b != NULL;
    if (!group_ok("kept", d->k_extent, d->k_a_stride, d->k_b_stride, d->k_ndim, two)) return -1;
    if (!group_ok("reduced", d->r_extent, d->r_a_stride, d->r_b_stride, d->r_ndim, two)) return -1;
    if (d->a == NULL) {
        snprintf(g_err, sizeof(g_err), "null pointer");
        return -1;
    }
    const uintptr_t sz = (uintptr_t)itemsize_of(d->dtype);
    if ((uintptr_t)d->a % sz || (uintptr_t)d->b % sz) {
        snprintf(g_err, sizeof(g_err), "source not aligned to its element size");
        return -1;
    }
    const int rl = d->r_ndim - 1, kl = d->k_ndim - 1;
    if (rl >= 0 && d->r_a_stride[rl] == 1 && (!two || d->r_b_stride[rl] == 1) && d->r_extent[rl] >= GTMI_REDUCE_SHORT_ROW)
        return GTMI_REDUCE_AXIS_SEGMENT;
    if (kl >= 0 && d->k_a_stride[kl] == 1 && (!two || d->k_b_stride[kl] == 1) && d->k_extent[kl] >= GTMI_REDUCE_SHORT_ROW)
        return GTMI_REDUCE_AXIS_LANE;
    return GTMI_REDUCE_AXIS_GENERIC;
}

extern "C" int gtmi_reduce_axis_path(const gtmi_reduce_axis_desc* desc) { return choose_path(desc); }

static bool whole_lines(const int64_t* as, const int64_t* bs, int nd, bool two, int64_t sz) {
    for (int i = 0; i < nd; ++i) {
        if ((as[i] * sz) % 16) return false;
        if (two && (bs[i] * sz) % 16) return false;
    }
    return true;
}

// 16-B accesses on the SEGMENT and LANE paths: every source's base has the same phase within a
// 16-B line and every stride but the row's is whole lines. Returns the phase in elements, -1 when
// they do not apply.
static int vector_head(const gtmi_reduce_axis_desc* d, int path) {
    const int64_t sz = itemsize_of(d->dtype);
    const bool two = d->b != NULL;
    const bool seg = path == GTMI_REDUCE_AXIS_SEGMENT;
    const int64_t row = seg ? d->r_extent[d->r_ndim - 1] : d->k_extent[d->k_ndim - 1];
    if (row * sz < 64) return -1;
    const uintptr_t pa = (uintptr_t)d->a % 16;
    if (two && (uintptr_t)d->b % 16 != pa) return -1;
    if (!whole_lines(d->k_a_stride, d->k_b_stride, d->k_ndim - (seg ? 0 : 1), two, sz)) return -1;
    if (!whole_lines(d->r_a_stride, d->r_b_stride, d->r_ndim - (seg ? 1 : 0), two, sz)) return -1;
    return (int)(pa / (uintptr_t)sz);
}

static int device_cus(void) {
    static int cus[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cus[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev] = n;
    }
    return cus[dev];
}

// Work items of one part (waves on SEGMENT and LANE, lanes on GENERIC) and the most parts with
// work in them.
static void geometry(const gtmi_reduce_axis_desc* d, int path, int64_t* items, int64_t* max_parts) {
    const int64_t cells = product_of(d->k_extent, d->k_ndim), nred = product_of(d->r_extent, d->r_ndim);
    const int head = path == GTMI_REDUCE_AXIS_GENERIC ? -1 : vector_head(d, path);
    const int64_t vec = head >= 0 ? 16 / itemsize_of(d->dtype) : 1, h = head >= 0 ? head : 0;
    if (path == GTMI_REDUCE_AXIS_SEGMENT) {
        const int64_t n = d->r_extent[d->r_ndim - 1], per = 64 * GTMI_AXIS_UNROLL;
        *items = cells;
        *max_parts = (nred / n) * (((h + n + vec - 1) / vec + per - 1) / per);
    } else if (path == GTMI_REDUCE_AXIS_LANE) {
        const int64_t nrow = d->k_extent[d->k_ndim - 1];
        *items = (cells / nrow) * (((h + nrow + vec - 1) / vec + 63) / 64);
        *max_parts = nred;
    } else {
        *items = cells;
        *max_parts = nred;
    }
}

extern "C" int gtmi_reduce_axis_parts(const gtmi_reduce_axis_desc* desc, int requested) {
    const int path = choose_path(desc);
    if (path < 0) return -1;
    if (requested > 0) return requested > GTMI_REDUCE_AXIS_MAX_PARTS ? GTMI_REDUCE_AXIS_MAX_PARTS : requested;
    int64_t items, max_parts;
    geometry(desc, path, &items, &max_parts);
    // What fills the chip: the grid's CUs * 8 blocks of 4 waves (lanes * 256 on GENERIC); on LANE the
    // 16 waves per CU its kernels' registers admit. The parts are rounded DOWN so that no wave gets
    // a second item: a wave walks its item at the latency of its own few loads in flight, and a
    // handful of waves with two items each would be a tail as long as the whole pass.
    const int64_t per_cu = path == GTMI_REDUCE_AXIS_GENERIC ? GTMI_AXIS_BLOCKS_PER_CU * GTMI_AXIS_THREADS
                           : path == GTMI_REDUCE_AXIS_LANE  ? GTMI_AXIS_LANE_WAVES_PER_CU
                                                            : GTMI_AXIS_BLOCKS_PER_CU * GTMI_AXIS_WAVES;
    const int64_t fill = (int64_t)device_cus() * per_cu;
    int64_t parts = fill / items;
    if (parts > max_parts) parts = max_parts;
    if (parts > GTMI_REDUCE_AXIS_MAX_PARTS) parts = GTMI_REDUCE_AXIS_MAX_PARTS;
    return (int)(parts < 1 ? 1 : parts);
}

static dim3 grid_for(int64_t work, int64_t per_block) {
    const int64_t cap = (int64_t)device_cus() * GTMI_AXIS_BLOCKS_PER_CU;
    int64_t blocks = (work + per_block - 1) / per_block;
    if (blocks > cap) blocks = cap;
    return dim3((unsigned)(blocks < 1 ? 1 : blocks));
}

template <typename T, bool TWO, typename Acc>
static void launch_pass(const gtmi_reduce_axis_desc* d, int path, Pass ps, uint64_t* ws, uint64_t* result, hipStream_t stream) {
    AxBox bx;
    memset(&bx, 0, sizeof(bx));
    bx.a = (const char*)d->a;
    bx.b = (const char*)d->b;
    bx.nk = d->k_ndim;
    bx.nr = d->r_ndim;
    for (int i = 0; i < d->k_ndim; ++i) {
        bx.kext[i] = d->k_extent[i];
        bx.kas[i] = d->k_a_stride[i];
        bx.kbs[i] = TWO ? d->k_b_stride[i] : 0;
    }
    for (int i = 0; i < d->r_ndim; ++i) {
        bx.rext[i] = d->r_extent[i];
        bx.ras[i] = d->r_a_stride[i];
        bx.rbs[i] = TWO ? d->r_b_stride[i] : 0;
    }
    bx.cells = product_of(d->k_extent, d->k_ndim);
    bx.nred = product_of(d->r_extent, d->r_ndim);
    const uint32_t mask = ps.mask;
    ps.final = ps.parts == 1;
    ps.out = ps.final ? result : ws;
    if (!ps.final) ps.mask = base_mask(mask);  // part records carry the base slots the mask is computed from
    int64_t items, max_parts;
    geometry(d, path, &items, &max_parts);
    const dim3 block(GTMI_AXIS_THREADS);
    constexpr int VEC = 16 / (int)sizeof(T);
    if (path == GTMI_REDUCE_AXIS_GENERIC) {
        ps.head = 0;
        hipLaunchKernelGGL((gtmi_axis_flat<T, TWO, Acc>), grid_for(items * ps.parts, GTMI_AXIS_THREADS), block, 0, stream, bx, ps);
    } else {
        const int head = vector_head(d, path);
        ps.head = head >= 0 ? head : 0;
        const dim3 grid = grid_for(items * ps.parts, GTMI_AXIS_WAVES);
        if (path == GTMI_REDUCE_AXIS_SEGMENT) {
            if (head >= 0)
                hipLaunchKernelGGL((gtmi_axis_segment<T, VEC, TWO, Acc>), grid, block, 0, stream, bx, ps);
            else
                hipLaunchKernelGGL((gtmi_axis_segment<T, 1, TWO, Acc>), grid, block, 0, stream, bx, ps);
        } else {
            if (head >= 0)
                hipLaunchKernelGGL((gtmi_axis_lane<T, VEC, TWO, Acc>), grid, block, 0, stream, bx, ps);
            else
                hipLaunchKernelGGL((gtmi_axis_lane<T, 1, TWO, Acc>), grid, block, 0, stream, bx, ps);
        }
    }
    if (!ps.final)
        hipLaunchKernelGGL((gtmi_axis_records<Acc>), grid_for(bx.cells, GTMI_AXIS_THREADS), block, 0, stream, (const uint64_t*)ws,
                           ps.parts, bx.cells, mask, base_mask(mask), result);
}

template <typename T, template <typename> class AccT>
static void launch_sources(const gtmi_reduce_axis_desc* d, int path, const Pass& ps, uint64_t* ws, uint64_t* result,
                           hipStream_t stream) {
    using Acc = AccT<typename Summand<T>::type>;
    if (d->b != NULL)
        launch_pass<T, true, Acc>(d, path, ps, ws, result, stream);
    else
        launch_pass<T, false, Acc>(d, path, ps, ws, result, stream);
}

static int launch_status(void) {
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString(err));
        return (int)err;
    }
    return 0;
}

template <template <typename> class AccT>
static int run_pass(const gtmi_reduce_axis_desc* d, Pass ps, void* workspace, void* result, void* stream_ptr) {
    const int path = choose_path(d);
    if (path < 0) return 1;
    if (result == NULL || (ps.parts > 1 && workspace == NULL)) {
        snprintf(g_err, sizeof(g_err), "null workspace or result");
        return 1;
    }
    if (ps.parts < 1 || ps.parts > GTMI_REDUCE_AXIS_MAX_PARTS) {
        snprintf(g_err, sizeof(g_err), "parts=%d outside [1, %d]", (int)ps.parts, GTMI_REDUCE_AXIS_MAX_PARTS);
        return 1;
    }
    hipStream_t stream = (hipStream_t)stream_ptr;
    uint64_t* ws = (uint64_t*)workspace;
    uint64_t* res = (uint64_t*)result;
    switch (d->dtype) {
        case GTMI_REDUCE_F32: launch_sources<float, AccT>(d, path, ps, ws, res, stream); break;
        case GTMI_REDUCE_F64: launch_sources<double, AccT>(d, path, ps, ws, res, stream); break;
        case GTMI_REDUCE_I32: launch_sources<int32_t, AccT>(d, path, ps, ws, res, stream); break;
        default: launch_sources<int64_t, AccT>(d, path, ps, ws, res, stream); break;
    }
    return launch_status();
}

extern "C" int gtmi_reduce_axis_scan(const gtmi_reduce_axis_desc* desc, uint32_t mask, void* workspace, void* result, int parts,
                                     void* stream) {
    GTMI_RANGE_PUSH("gtmi_reduce_axis_scan");
    Pass ps;
    memset(&ps, 0, sizeof(ps));
    ps.L = 1;
    ps.parts = parts;
    ps.mask = mask & ((1u << GTMI_REDUCE_SCAN_SLOTS) - 1u);
    const int rc = run_pass<ScanAcc>(desc, ps, workspace, result, stream);
    GTMI_RANGE_POP();
    return rc;
}

extern "C" int gtmi_reduce_axis_folds(const gtmi_reduce_axis_desc* desc, const void* m, int64_t n, void* workspace, void* result,
                                      int parts, void* stream) {
    g_err[0] = 0;
    if (m == NULL) {
        snprintf(g_err, sizeof(g_err), "null absolute maxima");
        return 1;
    }
    GTMI_RANGE_PUSH("gtmi_reduce_axis_folds");
    Pass ps;
    memset(&ps, 0, sizeof(ps));
    ps.m = (const double*)m;
    ps.L = ceil_log2_l(n);
    ps.parts = parts;
    const int rc = run_pass<FoldAcc>(desc, ps, workspace, result, stream);
    GTMI_RANGE_POP();
    return rc;
}

extern "C" int gtmi_reduce_axis_finish_sum(const void* scan, const void* folds, int64_t cells, int64_t n, int dtype, void* out,
                                           void* stream) {
    g_err[0] = 0;
    if (scan == NULL || folds == NULL || out == NULL || cells < 1 || dtype < GTMI_REDUCE_F32 || dtype > GTMI_REDUCE_I64) {
        snprintf(g_err, sizeof(g_err), "bad arguments to gtmi_reduce_axis_finish_sum");
        return 1;
    }
    const int floating = dtype == GTMI_REDUCE_F32 || dtype == GTMI_REDUCE_F64;
    hipLaunchKernelGGL(gtmi_axis_finish, grid_for(cells, GTMI_AXIS_THREADS), dim3(GTMI_AXIS_THREADS), 0, (hipStream_t)stream,
                       (const uint64_t*)scan, (const uint64_t*)folds, cells, ceil_log2_l(n), floating, (uint64_t*)out);
    return launch_status();
}

extern "C" int gtmi_reduce_axis_combine(const void* records, int nrec, int64_t cells, int dtype, uint32_t mask, void* result,
                                        void* stream) {
    g_err[0] = 0;
    if (records == NULL || result == NULL || nrec < 1 || cells < 1 || dtype < GTMI_REDUCE_F32 || dtype > GTMI_REDUCE_I64) {
        snprintf(g_err, sizeof(g_err), "bad arguments to gtmi_reduce_axis_combine");
        return 1;
    }
    mask &= (1u << GTMI_REDUCE_SCAN_SLOTS) - 1u;
    const dim3 grid = grid_for(cells, GTMI_AXIS_THREADS), block(GTMI_AXIS_THREADS);
    if (dtype == GTMI_REDUCE_F32 || dtype == GTMI_REDUCE_F64)
        hipLaunchKernelGGL((gtmi_axis_records<ScanAcc<double>>), grid, block, 0, (hipStream_t)stream, (const uint64_t*)records, nrec,
                           cells, mask, base_mask(mask), (uint64_t*)result);
    else
        hipLaunchKernelGGL((gtmi_axis_records<ScanAcc<int64_t>>), grid, block, 0, (hipStream_t)stream, (const uint64_t*)records,
                           nrec, cells, mask, base_mask(mask), (uint64_t*)result);
    return launch_status();
}
