// gtmi_relayout.hip -- one strided box copied between two device arrays of equal shape
// (storage.from_array / assign / contiguous; include/gtmi_relayout.h).
//
// The descriptor is canonical: dimensions ordered by the destination's stride, slowest first, so
// the last dimension is the destination's fastest. Three paths, chosen on the host:
//   ROW      both sides have stride 1 on the last dimension: a wave moves 64-lane chunks of it,
//            16 B per lane when both sides share their 16-B phase, else one element per lane;
//   TILE     the source has stride 1 on another dimension `a`: a 256-thread block stages a 64x64
//            tile of the (a, last) plane in LDS, reads rows along a, writes rows along the last
//            dimension -- both global sides coalesced;
//   GENERIC  everything else: one element per lane in destination-fastest order.
// Outer indices are decomposed once per wave (rows) or block (tiles) from wave-uniform values,
// as in the wide path of gtmi_halo.hip; rows shorter than GTMI_RELAYOUT_SHORT_ROW take one
// element per lane of a flat index instead (a wave per row would idle most lanes).
// All offsets are 64-bit. No atomics, no inter-block synchronisation, plain C++ stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "gtmi_roctx.h"

#include "gtmi_relayout.h"

#define GTMI_RELAYOUT_SHORT_ROW 32    // rows below this many elements go element-per-lane
#define GTMI_RELAYOUT_MAX_BLOCKS 4096 // grid-stride beyond: 16 blocks (64 waves) per CU
#define GTMI_RELAYOUT_TILE_DIM 64
#define GTMI_RELAYOUT_VEC_UNROLL 4    // 16-B ROW kernel: 64-lane chunks of a row per wave and trip (4 KB)

static thread_local char g_err[512];

struct Box {  // the descriptor as the kernels take it (by value)
    const char* src;
    char* dst;
    int64_t ext[GTMI_RELAYOUT_MAX_DIMS];
    int64_t ss[GTMI_RELAYOUT_MAX_DIMS];
    int64_t ds[GTMI_RELAYOUT_MAX_DIMS];
    int32_t ndim;
};

// Offsets of outer index `r` over the dimensions before `last`, skipping `skip_a` / `skip_b`.
__device__ __forceinline__ void outer_offsets(const Box& bx, int64_t r, int last, int skip_a, int skip_b, int64_t& so,
                                              int64_t& d_o) {
    so = 0;
    d_o = 0;
    for (int d = last - 1; d >= 0; --d) {
        if (d == skip_a || d == skip_b) continue;
        const int64_t e = bx.ext[d], q = r / e, idx = r - q * e;
        so += idx * bx.ss[d];
        d_o += idx * bx.ds[d];
        r = q;
    }
}

// One wave per (row, 64-element chunk of the last dimension); run-time strides on both sides
// (ROW without the 16-B phase: 1 and 1; GENERIC: anything, 0 on the source included).
template <typename T>
__global__ void __launch_bounds__(256) gtmi_relayout_rows(const Box bx) {
    const int lane = (int)(threadIdx.x & 63);
    const int last = bx.ndim - 1;
    const int64_t n = bx.ext[last], ssl = bx.ss[last], dsl = bx.ds[last];
    const int64_t cpr = (n + 63) / 64;
    int64_t rows = 1;
    for (int d = 0; d < last; ++d) rows *= bx.ext[d];
    const int64_t units = rows * cpr;
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x / 64);
    const int64_t w0 = (int64_t)blockIdx.x * (blockDim.x / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const T* __restrict__ src = (const T*)bx.src;
    T* __restrict__ dst = (T*)bx.dst;
    for (int64_t u = w0; u < units; u += nwaves) {
        const int64_t row = u / cpr, c = u - row * cpr;
        int64_t so, d_o;
        outer_offsets(bx, row, last, -1, -1, so, d_o);
        const int64_t i = c * 64 + lane;
        if (i < n) dst[d_o + i * dsl] = src[so + i * ssl];
    }
}

// The elements of the 16-B vector starting at row-relative element e0 that lie inside [0, n).
template <typename T>
__device__ __forceinline__ void copy_partial(T* __restrict__ drow, const T* __restrict__ srow, int64_t e0, int64_t n) {
    constexpr int V = 16 / (int)sizeof(T);
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const int64_t e = e0 + k;
        if (e >= 0 && e < n) drow[e] = srow[e];
    }
}

// ROW with 16-B accesses: both bases have the same phase `head` (in elements) within a 16-B
// line and every outer stride is a multiple of 16 B, so every row starts at that phase. A row
// is walked as the 16-B vectors of the line-aligned span that contains it; a vector that sticks
// out of the row (first and last one) goes element by element, so nothing outside is touched.
template <typename T>
__global__ void __launch_bounds__(256) gtmi_relayout_rows_vec(const Box bx, int head) {
    constexpr int V = 16 / (int)sizeof(T);
    const int lane = (int)(threadIdx.x & 63);
    const int last = bx.ndim - 1;
    const int64_t n = bx.ext[last];
    constexpr int U = GTMI_RELAYOUT_VEC_UNROLL;
    const int64_t nvec = (head + n + V - 1) / V;
    const int64_t cpr = (nvec + 64 * U - 1) / (64 * U);
    int64_t rows = 1;
    for (int d = 0; d < last; ++d) rows *= bx.ext[d];
    const int64_t units = rows * cpr;
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x / 64);
    const int64_t w0 = (int64_t)blockIdx.x * (blockDim.x / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const T* __restrict__ src = (const T*)bx.src;
    T* __restrict__ dst = (T*)bx.dst;
    for (int64_t u = w0; u < units; u += nwaves) {
        const int64_t row = u / cpr, c = u - row * cpr;
        int64_t so, d_o;
        outer_offsets(bx, row, last, -1, -1, so, d_o);
        // U chunks of the row per wave: the whole vectors first (loads, then stores), then the
        // at most two vectors per row that stick out of it
        // (scalars, not arrays: an array of U vectors was placed in LDS by the compiler)
        static_assert(U == 4, "the chunks of a trip are written out below");
        const int64_t ea = (c * U * 64 + lane) * V - head;  // first element of chunk 0's vector, relative to the row
        const int64_t eb = ea + 64 * V, ec = eb + 64 * V, ed = ec + 64 * V;
        const bool wa = ea >= 0 && ea + V <= n, wb = eb >= 0 && eb + V <= n;
        const bool wc = ec >= 0 && ec + V <= n, wd = ed >= 0 && ed + V <= n;
        uint4 ra = {}, rb = {}, rc = {}, rd = {};
        if (wa) ra = *(const uint4*)(src + so + ea);
        if (wb) rb = *(const uint4*)(src + so + eb);
        if (wc) rc = *(const uint4*)(src + so + ec);
        if (wd) rd = *(const uint4*)(src + so + ed);
        if (wa) *(uint4*)(dst + d_o + ea) = ra;
        if (wb) *(uint4*)(dst + d_o + eb) = rb;
        if (wc) *(uint4*)(dst + d_o + ec) = rc;
        if (wd) *(uint4*)(dst + d_o + ed) = rd;
        if (!wa) copy_partial<T>(dst + d_o, src + so, ea, n);
        if (!wb) copy_partial<T>(dst + d_o, src + so, eb, n);
        if (!wc) copy_partial<T>(dst + d_o, src + so, ec, n);
        if (!wd) copy_partial<T>(dst + d_o, src + so, ed, n);
    }
}

// One element per lane of the flat destination-order index (short rows). I is the index type of
// the decomposition: 32-bit when the box has at most 2^32 elements.
template <typename T, typename I>
__global__ void __launch_bounds__(256) gtmi_relayout_flat(const Box bx, int64_t total) {
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    const T* __restrict__ src = (const T*)bx.src;
    T* __restrict__ dst = (T*)bx.dst;
    for (int64_t el = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; el < total; el += nthreads) {
        I r = (I)el;
        int64_t so = 0, d_o = 0;
        for (int d = bx.ndim - 1; d >= 0; --d) {
            const I e = (I)bx.ext[d], q = r / e, idx = r - q * e;
            so += (int64_t)idx * bx.ss[d];
            d_o += (int64_t)idx * bx.ds[d];
            r = q;
        }
        dst[d_o] = src[so];
    }
}

// TILE: the source has stride 1 on dimension ia, the destination on dimension ib (the last).
// A block stages a 64x64 tile of the (ia, ib) plane: wave w loads rows w*16..w*16+15 along ia
// (row index = ib), then stores rows along ib (row index = ia) read as LDS columns. The pitch
// makes the column read conflict-free: lane l reads byte l*P*sizeof(T); for 8 B (ds_read_b64,
// 64 banks, 32-lane groups) P = 65 puts lane l on banks 2l, 2l+1 (mod 64); for 4 B P = 65
// dwords, for 2 B P = 66 (33 dwords) and for 1 B P = 68 (17 dwords) are odd dword pitches, so
// the 32 lanes of a group hit 32 different banks. Trip counts depend on blockIdx only and both
// barriers sit in block-uniform control flow; edge tiles are masked per element.
template <typename T>
__global__ void __launch_bounds__(256) gtmi_relayout_tile(const Box bx, int ia) {
    constexpr int TD = GTMI_RELAYOUT_TILE_DIM;
    constexpr int P = TD + (sizeof(T) >= 4 ? 1 : 4 / (int)sizeof(T));
    constexpr int RPW = TD / 4;  // rows per wave
    __shared__ T tile[TD * P];
    const int lane = (int)(threadIdx.x & 63);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int ib = bx.ndim - 1;
    const int64_t ea = bx.ext[ia], eb = bx.ext[ib], ssb = bx.ss[ib], dsa = bx.ds[ia];
    const int64_t ta = (ea + TD - 1) / TD, tb = (eb + TD - 1) / TD;
    int64_t outer = 1;
    for (int d = 0; d < ib; ++d)
        if (d != ia) outer *= bx.ext[d];
    const int64_t tiles = outer * ta * tb;
    const T* __restrict__ src = (const T*)bx.src;
    T* __restrict__ dst = (T*)bx.dst;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t q = t / ta, a0 = (t - q * ta) * TD;
        const int64_t o = q / tb, b0 = (q - o * tb) * TD;
        int64_t so, d_o;
        outer_offsets(bx, o, ib, ia, -1, so, d_o);
        T v[RPW];
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const int64_t a = a0 + lane, b = b0 + w * RPW + r;
            v[r] = (a < ea && b < eb) ? src[so + a + b * ssb] : (T)0;
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r) tile[(w * RPW + r) * P + lane] = v[r];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const int64_t a = a0 + w * RPW + r, b = b0 + lane;
            if (a < ea && b < eb) dst[d_o + a * dsa + b] = tile[lane * P + w * RPW + r];
        }
        __syncthreads();  // the next tile overwrites the stage
    }
}

extern "C" const char* gtmi_relayout_last_error(void) { return g_err; }
extern "C" int gtmi_relayout_abi_version(void) { return GTMI_RELAYOUT_ABI_VERSION; }

// Validates `d`; returns the path, -1 on error (g_err set), -2 for an empty box. *ia is the
// source's stride-1 dimension on the TILE path.
static int choose_path(const gtmi_relayout_desc* d, int* ia) {
    g_err[0] = 0;
    if (d == NULL || d->ndim < 1 || d->ndim > GTMI_RELAYOUT_MAX_DIMS) {
        snprintf(g_err, sizeof(g_err), "bad descriptor: ndim=%d", d ? (int)d->ndim : -1);
        return -1;
    }
    if (d->itemsize != 1 && d->itemsize != 2 && d->itemsize != 4 && d->itemsize != 8) {
        snprintf(g_err, sizeof(g_err), "bad descriptor: itemsize=%d", (int)d->itemsize);
        return -1;
    }
    bool empty = false;
    for (int i = 0; i < d->ndim; ++i) {
        if (d->extent[i] < 0 || d->src_stride[i] < 0 || d->dst_stride[i] <= 0) {
            snprintf(g_err, sizeof(g_err), "dimension %d: extent=%lld src_stride=%lld dst_stride=%lld", i,
                     (long long)d->extent[i], (long long)d->src_stride[i], (long long)d->dst_stride[i]);
            return -1;
        }
        if (d->extent[i] == 0) empty = true;
    }
    if (empty) return -2;
    for (int i = 0; i + 1 < d->ndim; ++i) {
        // slowest first, and no destination element written twice
        if (d->dst_stride[i] < d->dst_stride[i + 1] * d->extent[i + 1]) {
            snprintf(g_err, sizeof(g_err), "destination dimensions %d and %d overlap or are not ordered", i, i + 1);
            return -1;
        }
    }
    if (d->src == NULL || d->dst == NULL) {
        snprintf(g_err, sizeof(g_err), "null pointer");
        return -1;
    }
    const int last = d->ndim - 1;
    if (d->dst_stride[last] == 1 && d->src_stride[last] == 1) return GTMI_RELAYOUT_ROW;
    if (d->dst_stride[last] == 1 && d->extent[last] >= GTMI_RELAYOUT_TILE_MIN) {
        int a = -1;
        for (int i = 0; i < last; ++i)
            if (d->src_stride[i] == 1 && (a < 0 || d->extent[i] >= d->extent[a])) a = i;
        if (a >= 0 && d->extent[a] >= GTMI_RELAYOUT_TILE_MIN) {
            *ia = a;
            return GTMI_RELAYOUT_TILE;
        }
    }
    return GTMI_RELAYOUT_GENERIC;
}

extern "C" int gtmi_relayout_path(const gtmi_relayout_desc* desc) {
    int ia = -1;
    const int p = choose_path(desc, &ia);
    return p == -2 ? GTMI_RELAYOUT_ROW : p;
}

static unsigned capped_blocks(int64_t blocks) {
    if (blocks < 1) blocks = 1;
    return (unsigned)(blocks > GTMI_RELAYOUT_MAX_BLOCKS ? GTMI_RELAYOUT_MAX_BLOCKS : blocks);
}

template <typename T>
static void launch(const gtmi_relayout_desc* d, int path, int ia, hipStream_t stream) {
    Box bx;
    memset(&bx, 0, sizeof(bx));
    bx.src = (const char*)d->src;
    bx.dst = (char*)d->dst;
    bx.ndim = d->ndim;
    const int last = d->ndim - 1;
    int64_t rows = 1;
    for (int i = 0; i < d->ndim; ++i) {
        bx.ext[i] = d->extent[i];
        bx.ss[i] = d->src_stride[i];
        bx.ds[i] = d->dst_stride[i];
        if (i < last) rows *= d->extent[i];
    }
    const int64_t n = d->extent[last];
    if (path == GTMI_RELAYOUT_TILE) {
        const int64_t td = GTMI_RELAYOUT_TILE_DIM;
        const int64_t tiles = rows / d->extent[ia] * ((d->extent[ia] + td - 1) / td) * ((n + td - 1) / td);
        hipLaunchKernelGGL(gtmi_relayout_tile<T>, dim3(capped_blocks(tiles)), dim3(256), 0, stream, bx, ia);
        return;
    }
    if (path == GTMI_RELAYOUT_ROW && sizeof(T) < 16 && n * (int64_t)sizeof(T) >= 64) {
        // 16-B accesses: same phase of both bases within a 16-B line, outer strides whole lines
        const uintptr_t ps = (uintptr_t)d->src % 16, pd = (uintptr_t)d->dst % 16;
        bool ok = ps == pd && ps % sizeof(T) == 0;
        for (int i = 0; i < last && ok; ++i)
            ok = (d->src_stride[i] * (int64_t)sizeof(T)) % 16 == 0 && (d->dst_stride[i] * (int64_t)sizeof(T)) % 16 == 0;
        if (ok) {
            const int head = (int)(ps / sizeof(T));
            const int64_t V = 16 / (int64_t)sizeof(T);
            const int64_t per = 64 * GTMI_RELAYOUT_VEC_UNROLL;
            const int64_t cpr = ((head + n + V - 1) / V + per - 1) / per;
            hipLaunchKernelGGL(gtmi_relayout_rows_vec<T>, dim3(capped_blocks((rows * cpr + 3) / 4)), dim3(256), 0, stream,
                               bx, head);
            return;
        }
    }
    if (n >= GTMI_RELAYOUT_SHORT_ROW) {
        const int64_t cpr = (n + 63) / 64;
        hipLaunchKernelGGL(gtmi_relayout_rows<T>, dim3(capped_blocks((rows * cpr + 3) / 4)), dim3(256), 0, stream, bx);
        return;
    }
    const int64_t total = rows * n;
    const unsigned blocks = capped_blocks((total + 255) / 256);
    if (total <= 0xffffffffLL)
        hipLaunchKernelGGL((gtmi_relayout_flat<T, uint32_t>), dim3(blocks), dim3(256), 0, stream, bx, total);
    else
        hipLaunchKernelGGL((gtmi_relayout_flat<T, uint64_t>), dim3(blocks), dim3(256), 0, stream, bx, total);
}

static int relayout_copy_impl(const gtmi_relayout_desc* d, void* stream_ptr) {
    int ia = -1;
    const int path = choose_path(d, &ia);
    if (path == -2) return 0;
    if (path < 0) return 1;
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (d->itemsize == 8)
        launch<uint64_t>(d, path, ia, stream);
    else if (d->itemsize == 4)
        launch<uint32_t>(d, path, ia, stream);
    else if (d->itemsize == 2)
        launch<uint16_t>(d, path, ia, stream);
    else
        launch<uint8_t>(d, path, ia, stream);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "HIP launch failed: %s", hipGetErrorString(err));
        return (int)err;
    }
    return 0;
}

extern "C" int gtmi_relayout_copy(const gtmi_relayout_desc* desc, void* stream_ptr) {
    GTMI_RANGE_PUSH("gtmi_relayout");
    const int rc = relayout_copy_impl(desc, stream_ptr);
    GTMI_RANGE_POP();
    return rc;
}
