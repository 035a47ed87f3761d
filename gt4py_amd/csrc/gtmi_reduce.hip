// gtmi_reduce.hip -- reductions over one strided box of one or two device arrays
// (storage.reduce; include/gtmi_reduce.h). The numpy restatement in storage/reduce.py defines
// every result; this file follows it operation by operation.
//
// Two passes, each one launch over the box plus a one-block launch over the partial records:
//   scan   absolute maximum, minimum, maximum and the counts of NaN / +Inf / -Inf summands;
//   folds  three sums of the summands pre-rounded against C_f = 1.5 * 2^E_f (q = (r + C) - C,
//          S_f += q, r -= q): every q of a fold is a multiple of 2^(E_f - 52) and every partial
//          sum stays below 2^(E_f + 1), so each S_f is exact in f64 in ANY order. That is what
//          makes the grid size, the lane a summand lands on and the order of the partial
//          records irrelevant to the bits of the result. The file is built with
//          -ffp-contract=off and without fast-math: (r + C) - C is two IEEE operations.
// The descriptor is canonical: the last dimension is the first source's fastest. Two paths,
// chosen on the host:
//   ROW      stride 1 on the last dimension in every source: a wave owns 64-lane chunks of a row,
//            16 B per lane when every row of every source starts at the same phase of a 16-B
//            line (vectors that stick out of the row go element by element, so nothing outside
//            the box is read), else one element per lane; outer indices are decomposed once per
//            wave and trip from wave-uniform values, as in gtmi_halo.hip and gtmi_relayout.hip;
//   GENERIC  any other stride, and rows shorter than GTMI_REDUCE_SHORT_ROW: one element per lane
//            of the flat index.
// Per lane, then across the wave with gtmi::shfl, then across the block's four waves through
// LDS; one record per block, plain stores. No atomics, no inter-block protocol, no host
// synchronisation. All offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "gtmi_device.h"
#include "gtmi_roctx.h"

#include "gtmi_reduce.h"
#include "gtmi_reduce_rules.h"  // summands, scan update, fold plan, fold step, finish

#define GTMI_REDUCE_UNROLL 4         // ROW kernel: 64-lane chunks of a row per wave and trip
#define GTMI_REDUCE_BLOCKS_PER_CU 8  // persistent grid: 32 waves per CU
#define GTMI_REDUCE_THREADS 256

static thread_local char g_err[512];

struct Box {  // the descriptor as the kernels take it (by value)
    const char* a;
    const char* b;
    int64_t ext[GTMI_REDUCE_MAX_DIMS];
    int64_t as[GTMI_REDUCE_MAX_DIMS];
    int64_t bs[GTMI_REDUCE_MAX_DIMS];
    int32_t ndim;
};

// Every lane's accumulator into one record at `out` (thread 0 writes). All 256 threads call it
// from block-uniform control flow.
template <typename Acc, bool FINAL> GTMI_DEV void block_reduce(Acc& acc, uint64_t* out) {
    __shared__ uint64_t stage[(GTMI_REDUCE_THREADS / 64) * Acc::SLOTS];
#pragma unroll
    for (int delta = 32; delta >= 1; delta >>= 1) {
        const Acc o = acc.shuffled(delta);
        acc.combine(o);
    }
    const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6);
    if (lane == 0) acc.store(stage + w * Acc::SLOTS);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < GTMI_REDUCE_THREADS / 64; ++k) {
            Acc o;
            o.load(stage + k * Acc::SLOTS);
            acc.combine(o);
        }
        if constexpr (FINAL)
            acc.finish(out);
        else
            acc.store(out);
    }
}

// ------------------------------------------------------------------ kernels
// Offsets of outer index `r` over the dimensions before `last`.
GTMI_DEV void outer_offsets(const Box& bx, int64_t r, int last, int64_t& oa, int64_t& ob) {
    oa = 0;
    ob = 0;
    for (int d = last - 1; d >= 0; --d) {
        const int64_t e = bx.ext[d], q = r / e, idx = r - q * e;
        oa += idx * bx.as[d];
        ob += idx * bx.bs[d];
        r = q;
    }
}

// ROW. VEC elements per lane and access: 16 / sizeof(T) when every row of every source starts
// `head` elements past a 16-B line (the row is walked as the vectors of the line-aligned span
// that contains it), else 1 with head 0.
template <typename T, int VEC, bool TWO, typename Acc>
__global__ void __launch_bounds__(GTMI_REDUCE_THREADS) gtmi_reduce_rows(const Box bx, int head, typename Acc::Ctx ctx,
                                                                      uint64_t* __restrict__ ws) {
    using Vt = gtmi::evec<T, VEC>;
    constexpr int U = GTMI_REDUCE_UNROLL;
    const int lane = (int)(threadIdx.x & 63);
    const int last = bx.ndim - 1;
    const int64_t n = bx.ext[last];
    const int64_t nvec = (head + n + VEC - 1) / VEC;
    const int64_t cpr = (nvec + 64 * U - 1) / (64 * U);
    int64_t rows = 1;
    for (int d = 0; d < last; ++d) rows *= bx.ext[d];
    const int64_t units = rows * cpr;
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x / 64);
    const int64_t w0 = (int64_t)blockIdx.x * (blockDim.x / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const T* __restrict__ a = (const T*)bx.a;
    const T* __restrict__ b = (const T*)bx.b;
    const typename Acc::Params prm(ctx);
    Acc acc;
    acc.init();
    for (int64_t u = w0; u < units; u += nwaves) {
        const int64_t row = u / cpr, c = u - row * cpr;
        int64_t oa, ob;
        outer_offsets(bx, row, last, oa, ob);
        const T* __restrict__ ra = a + oa;
        const T* __restrict__ rb = TWO ? b + ob : nullptr;
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
    block_reduce<Acc, false>(acc, ws + (int64_t)blockIdx.x * Acc::SLOTS);
}

// GENERIC: one element per lane of the flat index, any strides (0 included).
template <typename T, bool TWO, typename Acc>
__global__ void __launch_bounds__(GTMI_REDUCE_THREADS) gtmi_reduce_flat(const Box bx, int64_t total, typename Acc::Ctx ctx,
                                                                      uint64_t* __restrict__ ws) {
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    const T* __restrict__ a = (const T*)bx.a;
    const T* __restrict__ b = (const T*)bx.b;
    const typename Acc::Params prm(ctx);
    Acc acc;
    acc.init();
    for (int64_t el = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; el < total; el += nthreads) {
        int64_t r = el, oa = 0, ob = 0;
        for (int d = bx.ndim - 1; d >= 0; --d) {
            const int64_t e = bx.ext[d], q = r / e, idx = r - q * e;
            oa += idx * bx.as[d];
            ob += idx * bx.bs[d];
            r = q;
        }
        if constexpr (TWO)
            acc.add(product(summand(a[oa]), summand(b[ob])), prm);
        else
            acc.add(summand(a[oa]), prm);
    }
    block_reduce<Acc, false>(acc, ws + (int64_t)blockIdx.x * Acc::SLOTS);
}

// The partial records into the result (one block).
template <typename Acc>
__global__ void __launch_bounds__(GTMI_REDUCE_THREADS) gtmi_reduce_records(const uint64_t* __restrict__ ws, int nrec,
                                                                         uint64_t* __restrict__ result) {
    Acc acc;
    acc.init();
    for (int i = (int)threadIdx.x; i < nrec; i += GTMI_REDUCE_THREADS) {
        Acc o;
        o.load(ws + (int64_t)i * Acc::SLOTS);
        acc.combine(o);
    }
    block_reduce<Acc, true>(acc, result);
}

__global__ void gtmi_reduce_finish(const uint64_t* __restrict__ scan, const uint64_t* __restrict__ folds, int L,
                                   int floating, uint64_t* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (!floating) {
        out[0] = folds[0];
        return;
    }
    const int64_t nan = (int64_t)scan[GTMI_REDUCE_SCAN_NAN], pinf = (int64_t)scan[GTMI_REDUCE_SCAN_PINF];
    const int64_t ninf = (int64_t)scan[GTMI_REDUCE_SCAN_NINF];
    const double M = double_of(scan[GTMI_REDUCE_SCAN_ABSMAX]);
    out[0] = bits_of(finish_sum(nan, pinf, ninf, M, double_of(folds[0]), double_of(folds[1]), double_of(folds[2]), L));
}

// ------------------------------------------------------------------ host side
extern "C" const char* gtmi_reduce_last_error(void) { return g_err; }
extern "C" int gtmi_reduce_abi_version(void) { return GTMI_REDUCE_ABI_VERSION; }

static int itemsize_of(int dtype) { return (dtype == GTMI_REDUCE_F32 || dtype == GTMI_REDUCE_I32) ? 4 : 8; }

// Validates `d`; returns the path, -1 on error (g_err set), -2 for an empty box.
static int choose_path(const gtmi_reduce_desc* d) {
    g_err[0] = 0;
    if (d == NULL || d->ndim < 1 || d->ndim > GTMI_REDUCE_MAX_DIMS) {
        snprintf(g_err, sizeof(g_err), "bad descriptor: ndim=%d", d ? (int)d->ndim : -1);
        return -1;
    }
    if (d->dtype < GTMI_REDUCE_F32 || d->dtype > GTMI_REDUCE_I64) {
        snprintf(g_err, sizeof(g_err), "bad descriptor: dtype=%d", (int)d->dtype);
        return -1;
    }
    bool empty = false;
    for (int i = 0; i < d->ndim; ++i) {
        if (d->extent[i] < 0 || d->a_stride[i] < 0 || (d->b != NULL && d->b_stride[i] < 0)) {
            snprintf(g_err, sizeof(g_err), "dimension %d: extent=%lld a_stride=%lld b_stride=%lld", i,
                     (long long)d->extent[i], (long long)d->a_stride[i], (long long)d->b_stride[i]);
            return -1;
        }
        if (d->extent[i] == 0) empty = true;
    }
    if (empty) return -2;
    if (d->a == NULL) {
        snprintf(g_err, sizeof(g_err), "null pointer");
        return -1;
    }
    const uintptr_t sz = (uintptr_t)itemsize_of(d->dtype);
    if ((uintptr_t)d->a % sz || (uintptr_t)d->b % sz) {
        snprintf(g_err, sizeof(g_err), "source not aligned to its element size");
        return -1;
    }
    const int last = d->ndim - 1;
    if (d->a_stride[last] == 1 && (d->b == NULL || d->b_stride[last] == 1) && d->extent[last] >= GTMI_REDUCE_SHORT_ROW)
        return GTMI_REDUCE_ROW;
    return GTMI_REDUCE_GENERIC;
}

extern "C" int gtmi_reduce_path(const gtmi_reduce_desc* desc) {
    const int p = choose_path(desc);
    return p == -2 ? GTMI_REDUCE_GENERIC : p;
}

// 16-B accesses on the ROW path: every source's base has the same phase within a 16-B line and
// every outer stride is whole lines. Returns the phase in elements, -1 when they do not apply.
static int vector_head(const gtmi_reduce_desc* d) {
    const int64_t sz = itemsize_of(d->dtype);
    const int last = d->ndim - 1;
    if (d->extent[last] * sz < 64) return -1;
    const uintptr_t pa = (uintptr_t)d->a % 16;
    if (d->b != NULL && (uintptr_t)d->b % 16 != pa) return -1;
    for (int i = 0; i < last; ++i) {
        if ((d->a_stride[i] * sz) % 16) return -1;
        if (d->b != NULL && (d->b_stride[i] * sz) % 16) return -1;
    }
    return (int)(pa / (uintptr_t)sz);
}

// Blocks with work in them for `d` on `path`.
static int64_t blocks_needed(const gtmi_reduce_desc* d, int path) {
    const int last = d->ndim - 1;
    int64_t rows = 1;
    for (int i = 0; i < last; ++i) rows *= d->extent[i];
    const int64_t n = d->extent[last];
    if (path == GTMI_REDUCE_ROW) {
        const int head = vector_head(d);
        const int64_t vec = head >= 0 ? 16 / itemsize_of(d->dtype) : 1;
        const int64_t per = 64 * GTMI_REDUCE_UNROLL;
        const int64_t cpr = (((head >= 0 ? head : 0) + n + vec - 1) / vec + per - 1) / per;
        return (rows * cpr + 3) / 4;
    }
    return (rows * n + GTMI_REDUCE_THREADS - 1) / GTMI_REDUCE_THREADS;
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

extern "C" int gtmi_reduce_blocks(const gtmi_reduce_desc* desc, int requested) {
    const int path = choose_path(desc);
    if (path == -1) return -1;
    if (requested > 0) return requested > GTMI_REDUCE_MAX_BLOCKS ? GTMI_REDUCE_MAX_BLOCKS : requested;
    if (path == -2) return 1;
    const int64_t need = blocks_needed(desc, path);
    const int64_t cap = (int64_t)device_cus() * GTMI_REDUCE_BLOCKS_PER_CU;
    int64_t blocks = need < cap ? need : cap;
    if (blocks > GTMI_REDUCE_MAX_BLOCKS) blocks = GTMI_REDUCE_MAX_BLOCKS;
    return (int)(blocks < 1 ? 1 : blocks);
}

template <typename T, bool TWO, typename Acc>
static void launch_pass(const gtmi_reduce_desc* d, int path, typename Acc::Ctx ctx, uint64_t* ws, uint64_t* result,
                        int blocks, hipStream_t stream) {
    Box bx;
    memset(&bx, 0, sizeof(bx));
    bx.a = (const char*)d->a;
    bx.b = (const char*)d->b;
    bx.ndim = d->ndim;
    int64_t total = 1;
    for (int i = 0; i < d->ndim; ++i) {
        bx.ext[i] = d->extent[i];
        bx.as[i] = d->a_stride[i];
        bx.bs[i] = TWO ? d->b_stride[i] : 0;
        total *= d->extent[i];
    }
    const dim3 grid((unsigned)blocks), block(GTMI_REDUCE_THREADS);
    if (path == GTMI_REDUCE_ROW) {
        const int head = vector_head(d);
        constexpr int VEC = 16 / (int)sizeof(T);
        if (head >= 0)
            hipLaunchKernelGGL((gtmi_reduce_rows<T, VEC, TWO, Acc>), grid, block, 0, stream, bx, head, ctx, ws);
        else
            hipLaunchKernelGGL((gtmi_reduce_rows<T, 1, TWO, Acc>), grid, block, 0, stream, bx, 0, ctx, ws);
    } else {
        hipLaunchKernelGGL((gtmi_reduce_flat<T, TWO, Acc>), grid, block, 0, stream, bx, total, ctx, ws);
    }
    hipLaunchKernelGGL((gtmi_reduce_records<Acc>), dim3(1), block, 0, stream, (const uint64_t*)ws, blocks, result);
}

template <typename T, template <typename> class AccT>
static void launch_sources(const gtmi_reduce_desc* d, int path, typename AccT<typename Summand<T>::type>::Ctx ctx,
                           uint64_t* ws, uint64_t* result, int blocks, hipStream_t stream) {
    using Acc = AccT<typename Summand<T>::type>;
    if (d->b != NULL)
        launch_pass<T, true, Acc>(d, path, ctx, ws, result, blocks, stream);
    else
        launch_pass<T, false, Acc>(d, path, ctx, ws, result, blocks, stream);
}

template <template <typename> class AccT, typename Ctx>
static int run_pass(const gtmi_reduce_desc* d, Ctx ctx, void* workspace, void* result, int blocks, void* stream_ptr) {
    int path = choose_path(d);
    if (path == -1) return 1;
    if (workspace == NULL || result == NULL) {
        snprintf(g_err, sizeof(g_err), "null workspace or result");
        return 1;
    }
    if (blocks < 1 || blocks > GTMI_REDUCE_MAX_BLOCKS) {
        snprintf(g_err, sizeof(g_err), "blocks=%d outside [1, %d]", blocks, GTMI_REDUCE_MAX_BLOCKS);
        return 1;
    }
    hipStream_t stream = (hipStream_t)stream_ptr;
    uint64_t* ws = (uint64_t*)workspace;
    uint64_t* res = (uint64_t*)result;
    gtmi_reduce_desc e = *d;
    if (path == -2) {  // an empty box: the identities, through the same two launches over no element
        e.ndim = 1;
        e.extent[0] = 0;
        e.a_stride[0] = e.b_stride[0] = 1;
        path = GTMI_REDUCE_GENERIC;
    }
    switch (e.dtype) {
        case GTMI_REDUCE_F32: launch_sources<float, AccT>(&e, path, ctx, ws, res, blocks, stream); break;
        case GTMI_REDUCE_F64: launch_sources<double, AccT>(&e, path, ctx, ws, res, blocks, stream); break;
        case GTMI_REDUCE_I32: launch_sources<int32_t, AccT>(&e, path, ctx, ws, res, blocks, stream); break;
        default: launch_sources<int64_t, AccT>(&e, path, ctx, ws, res, blocks, stream); break;
    }
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString(err));
        return (int)err;
    }
    return 0;
}

extern "C" int gtmi_reduce_scan(const gtmi_reduce_desc* desc, void* workspace, void* result, int blocks, void* stream) {
    GTMI_RANGE_PUSH("gtmi_reduce_scan");
    const int rc = run_pass<ScanAcc>(desc, NoCtx{}, workspace, result, blocks, stream);
    GTMI_RANGE_POP();
    return rc;
}

extern "C" int gtmi_reduce_folds(const gtmi_reduce_desc* desc, const void* m, int64_t n, void* workspace, void* result,
                                 int blocks, void* stream) {
    g_err[0] = 0;
    if (m == NULL) {
        snprintf(g_err, sizeof(g_err), "null absolute maximum");
        return 1;
    }
    GTMI_RANGE_PUSH("gtmi_reduce_folds");
    FoldCtx ctx;
    ctx.m = (const double*)m;
    ctx.L = ceil_log2_l(n);
    const int rc = run_pass<FoldAcc>(desc, ctx, workspace, result, blocks, stream);
    GTMI_RANGE_POP();
    return rc;
}

extern "C" int gtmi_reduce_finish_sum(const void* scan, const void* folds, int64_t n, int dtype, void* out, void* stream) {
    g_err[0] = 0;
    if (scan == NULL || folds == NULL || out == NULL || dtype < GTMI_REDUCE_F32 || dtype > GTMI_REDUCE_I64) {
        snprintf(g_err, sizeof(g_err), "bad arguments to gtmi_reduce_finish_sum");
        return 1;
    }
    const int floating = dtype == GTMI_REDUCE_F32 || dtype == GTMI_REDUCE_F64;
    hipLaunchKernelGGL(gtmi_reduce_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, (const uint64_t*)scan,
                       (const uint64_t*)folds, ceil_log2_l(n), floating, (uint64_t*)out);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString(err));
        return (int)err;
    }
    return 0;
}

extern "C" int gtmi_reduce_combine(const void* records, int nrec, int dtype, void* result, void* stream) {
    g_err[0] = 0;
    if (records == NULL || result == NULL || nrec < 1 || dtype < GTMI_REDUCE_F32 || dtype > GTMI_REDUCE_I64) {
        snprintf(g_err, sizeof(g_err), "bad arguments to gtmi_reduce_combine");
        return 1;
    }
    if (dtype == GTMI_REDUCE_F32 || dtype == GTMI_REDUCE_F64)
        hipLaunchKernelGGL((gtmi_reduce_records<ScanAcc<double>>), dim3(1), dim3(GTMI_REDUCE_THREADS), 0, (hipStream_t)stream,
                           (const uint64_t*)records, nrec, (uint64_t*)result);
    else
        hipLaunchKernelGGL((gtmi_reduce_records<ScanAcc<int64_t>>), dim3(1), dim3(GTMI_REDUCE_THREADS), 0, (hipStream_t)stream,
                           (const uint64_t*)records, nrec, (uint64_t*)result);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString(err));
        return (int)err;
    }
    return 0;
}
