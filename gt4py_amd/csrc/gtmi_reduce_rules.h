// gtmi_reduce_rules.h -- the per-summand rules of storage.reduce, shared by gtmi_reduce.hip (one
// result per box) and gtmi_reduce_axis.hip (one result per kept cell): summands and products, the
// scan update, the fold plan from (M, L), the fold step and the finish. The numpy restatement in
// storage/reduce.py defines every result; this file follows it operation by operation. Both
// libraries carry this file's digest in their build keys.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "gtmi_device.h"

#include "gtmi_reduce.h"

#define GTMI_REDUCE_SHORT_ROW 32  // rows below this many elements go element-per-lane

// ------------------------------------------------------------------ summands
template <typename T> struct Summand { using type = int64_t; };
template <> struct Summand<float> { using type = double; };
template <> struct Summand<double> { using type = double; };

GTMI_DEV double summand(float a) { return (double)a; }
GTMI_DEV double summand(double a) { return a; }
GTMI_DEV int64_t summand(int32_t a) { return (int64_t)a; }
GTMI_DEV int64_t summand(int64_t a) { return a; }
GTMI_DEV double product(double a, double b) { return a * b; }  // one IEEE multiply (no contraction)
GTMI_DEV int64_t product(int64_t a, int64_t b) { return (int64_t)((uint64_t)a * (uint64_t)b); }

GTMI_DEV uint64_t bits_of(double v) {
    uint64_t u;
    __builtin_memcpy(&u, &v, 8);
    return u;
}
GTMI_DEV uint64_t bits_of(int64_t v) { return (uint64_t)v; }
GTMI_DEV double double_of(uint64_t u) {
    double v;
    __builtin_memcpy(&v, &u, 8);
    return v;
}
template <typename V> GTMI_DEV V value_of(uint64_t u);
template <> GTMI_DEV double value_of<double>(uint64_t u) { return double_of(u); }
template <> GTMI_DEV int64_t value_of<int64_t>(uint64_t u) { return (int64_t)u; }

// ------------------------------------------------------------------ the fold plan
// 2^k for k in [-1022, 1023]
GTMI_DEV double pow2(int k) { return double_of((uint64_t)(k + 1023) << 52); }

// The constants of the three folds for the absolute maximum M and L = max(1, ceil(log2 N))
// (storage/reduce.py fold_plan, same text).
struct FoldPlan {
    double c[3];
    double scale, unscale;
    int ident[3];  // the fold's grid lies below 2^-1074: q = r
    int zero;      // M is 0 or not finite: every fold sum is 0
};

GTMI_DEV FoldPlan fold_plan(double M, int L) {
    FoldPlan p;
    p.scale = p.unscale = 1.0;
    p.zero = 0;
    for (int f = 0; f < 3; ++f) {
        p.c[f] = 0.0;
        p.ident[f] = 0;
    }
    if (!(M > 0.0) || M == __builtin_inf()) {
        p.zero = 1;
        return p;
    }
    const uint64_t bits = bits_of(M);
    const int biased = (int)((bits >> 52) & 0x7ff);
    // M = m * 2^e with m in [0.5, 1)
    const int e = biased ? biased - 1022 : 64 - (int)__builtin_clzll(bits & 0xfffffffffffffULL) - 1074;
    int E = e + L;
    if (E > 1022) {  // huge M: scale the summands by 2^(1022 - E0), exactly
        p.scale = pow2(1022 - E);
        p.unscale = pow2(E - 1022);
        E = 1022;
    }
    for (int f = 0; f < 3; ++f) {
        if (E < -1022)
            p.ident[f] = 1;
        else
            p.c[f] = 1.5 * pow2(E);
        E = E - 52 + L;
    }
    return p;
}

static int ceil_log2_l(int64_t n) {  // L = max(1, ceil(log2 n))
    int l = 0;
    while (l < 63 && ((int64_t)1 << l) < n) ++l;
    return l < 1 ? 1 : l;
}

// ------------------------------------------------------------------ accumulators
// -0.0 orders below +0.0 (NaN never gets here)
GTMI_DEV bool less_total(double a, double b) { return a < b || (a == b && bits_of(a) > bits_of(b)); }
GTMI_DEV bool less_total(int64_t a, int64_t b) { return a < b; }

struct NoCtx {};

template <typename V> struct ScanAcc {
    static constexpr int SLOTS = GTMI_REDUCE_SCAN_SLOTS;
    static constexpr bool F = std::is_floating_point<V>::value;
    using Ctx = NoCtx;
    struct Params {
        GTMI_DEV explicit Params(const Ctx&) {}
        GTMI_DEV Params(double, int) {}
        GTMI_DEV Params() {}
    };
    V absmax, mn, mx;
    int64_t nan, pinf, ninf;

    GTMI_DEV void init() {
        if constexpr (F) {
            absmax = 0.0;
            mn = __builtin_inf();
            mx = -__builtin_inf();
        } else {
            absmax = INT64_MIN;  // |INT64_MIN| wraps to itself in int64, as numpy's abs does
            mn = INT64_MAX;
            mx = INT64_MIN;
        }
        nan = pinf = ninf = 0;
    }
    GTMI_DEV void add(V v, const Params&) {
        if constexpr (F) {
            if (v != v) {
                ++nan;
                return;
            }
            const double a = __builtin_fabs(v);
            absmax = a > absmax ? a : absmax;
            pinf += (v == __builtin_inf());
            ninf += (v == -__builtin_inf());
        } else {
            const int64_t a = v < 0 ? (int64_t)(0 - (uint64_t)v) : v;
            absmax = a > absmax ? a : absmax;
        }
        mn = less_total(v, mn) ? v : mn;
        mx = less_total(mx, v) ? v : mx;
    }
    GTMI_DEV void combine(const ScanAcc& o) {
        absmax = o.absmax > absmax ? o.absmax : absmax;
        mn = less_total(o.mn, mn) ? o.mn : mn;
        mx = less_total(mx, o.mx) ? o.mx : mx;
        nan += o.nan;
        pinf += o.pinf;
        ninf += o.ninf;
    }
    GTMI_DEV ScanAcc shuffled(int delta) const {
        ScanAcc o;
        o.absmax = gtmi::shfl(absmax, delta);
        o.mn = gtmi::shfl(mn, delta);
        o.mx = gtmi::shfl(mx, delta);
        o.nan = gtmi::shfl(nan, delta);
        o.pinf = gtmi::shfl(pinf, delta);
        o.ninf = gtmi::shfl(ninf, delta);
        return o;
    }
    template <typename P> GTMI_DEV void store(P* r) const {  // P: uint64_t in global memory or LDS
        r[GTMI_REDUCE_SCAN_ABSMAX] = bits_of(absmax);
        r[GTMI_REDUCE_SCAN_MIN] = bits_of(mn);
        r[GTMI_REDUCE_SCAN_MAX] = bits_of(mx);
        r[GTMI_REDUCE_SCAN_NAN] = (uint64_t)nan;
        r[GTMI_REDUCE_SCAN_PINF] = (uint64_t)pinf;
        r[GTMI_REDUCE_SCAN_NINF] = (uint64_t)ninf;
    }
    template <typename P> GTMI_DEV void load(const P* r) {
        absmax = value_of<V>(r[GTMI_REDUCE_SCAN_ABSMAX]);
        mn = value_of<V>(r[GTMI_REDUCE_SCAN_MIN]);
        mx = value_of<V>(r[GTMI_REDUCE_SCAN_MAX]);
        nan = (int64_t)r[GTMI_REDUCE_SCAN_NAN];
        pinf = (int64_t)r[GTMI_REDUCE_SCAN_PINF];
        ninf = (int64_t)r[GTMI_REDUCE_SCAN_NINF];
    }
    // the result record: the partial record's slots plus the derived ones
    GTMI_DEV void finish(uint64_t* r) const {
        store(r);
        r[GTMI_REDUCE_SCAN_NONFINITE] = (uint64_t)(nan + pinf + ninf);
        r[7] = 0;
        if constexpr (F) {
            const uint64_t qnan = 0x7ff8000000000000ULL;
            r[GTMI_REDUCE_SCAN_ABSMAX_NAN] = nan ? qnan : bits_of(absmax);
            r[GTMI_REDUCE_SCAN_MIN_NAN] = nan ? qnan : bits_of(mn);
            r[GTMI_REDUCE_SCAN_MAX_NAN] = nan ? qnan : bits_of(mx);
        } else {
            r[GTMI_REDUCE_SCAN_ABSMAX_NAN] = bits_of(absmax);
            r[GTMI_REDUCE_SCAN_MIN_NAN] = bits_of(mn);
            r[GTMI_REDUCE_SCAN_MAX_NAN] = bits_of(mx);
        }
        r[11] = 0;
    }
};

struct FoldCtx {
    const double* m;  // device memory
    int L;
};

template <typename V> struct FoldAcc;

template <> struct FoldAcc<double> {
    static constexpr int SLOTS = GTMI_REDUCE_FOLD_SLOTS;
    using Ctx = FoldCtx;
    struct Params {
        FoldPlan p;
        GTMI_DEV explicit Params(const Ctx& c) : p(fold_plan(*c.m, c.L)) {}
        GTMI_DEV Params(double M, int L) : p(fold_plan(M, L)) {}
        GTMI_DEV Params() {}
    };
    double s0, s1, s2;

    GTMI_DEV void init() { s0 = s1 = s2 = 0.0; }
    GTMI_DEV void add(double v, const Params& pp) {
        const FoldPlan& p = pp.p;
        if (p.zero) return;
        if (!(__builtin_fabs(v) < __builtin_inf())) v = 0.0;  // non-finite summands count as 0
        double r = v * p.scale;
        double q = p.ident[0] ? r : (r + p.c[0]) - p.c[0];
        s0 += q;
        r -= q;
        q = p.ident[1] ? r : (r + p.c[1]) - p.c[1];
        s1 += q;
        r -= q;
        q = p.ident[2] ? r : (r + p.c[2]) - p.c[2];
        s2 += q;
    }
    GTMI_DEV void combine(const FoldAcc& o) {
        s0 += o.s0;
        s1 += o.s1;
        s2 += o.s2;
    }
    GTMI_DEV FoldAcc shuffled(int delta) const {
        FoldAcc o;
        o.s0 = gtmi::shfl(s0, delta);
        o.s1 = gtmi::shfl(s1, delta);
        o.s2 = gtmi::shfl(s2, delta);
        return o;
    }
    template <typename P> GTMI_DEV void store(P* r) const {
        r[0] = bits_of(s0);
        r[1] = bits_of(s1);
        r[2] = bits_of(s2);
        r[3] = 0;
    }
    template <typename P> GTMI_DEV void load(const P* r) {
        s0 = double_of(r[0]);
        s1 = double_of(r[1]);
        s2 = double_of(r[2]);
    }
    GTMI_DEV void finish(uint64_t* r) const { store(r); }
};

template <> struct FoldAcc<int64_t> {  // int64 with wrap-around: one sum, S1 = S2 = 0
    static constexpr int SLOTS = GTMI_REDUCE_FOLD_SLOTS;
    using Ctx = FoldCtx;
    struct Params {
        GTMI_DEV explicit Params(const Ctx&) {}
        GTMI_DEV Params(double, int) {}
        GTMI_DEV Params() {}
    };
    uint64_t s0;

    GTMI_DEV void init() { s0 = 0; }
    GTMI_DEV void add(int64_t v, const Params&) { s0 += (uint64_t)v; }
    GTMI_DEV void combine(const FoldAcc& o) { s0 += o.s0; }
    GTMI_DEV FoldAcc shuffled(int delta) const {
        FoldAcc o;
        o.s0 = (uint64_t)gtmi::shfl((int64_t)s0, delta);
        return o;
    }
    template <typename P> GTMI_DEV void store(P* r) const {
        r[0] = s0;
        r[1] = r[2] = r[3] = 0;
    }
    template <typename P> GTMI_DEV void load(const P* r) { s0 = r[0]; }
    GTMI_DEV void finish(uint64_t* r) const { store(r); }
};

// ------------------------------------------------------------------ the finish
// The float sum from the scan's counts and absolute maximum and the three fold sums: the
// non-finite rules, +0.0 for M == 0, else S0 + (S1 + S2) scaled back (_finish_sum_host).
GTMI_DEV double finish_sum(int64_t nan, int64_t pinf, int64_t ninf, double M, double s0, double s1, double s2, int L) {
    if (nan > 0 || (pinf > 0 && ninf > 0)) return double_of(0x7ff8000000000000ULL);
    if (pinf > 0) return __builtin_inf();
    if (ninf > 0) return -__builtin_inf();
    if (M == 0.0) return 0.0;
    const FoldPlan p = fold_plan(M, L);
    return (s0 + (s1 + s2)) * p.unscale;
}
