// lbm_device.hpp -- device-side D2Q9 operators shared by every kernel of liblbm_hip.
//
// Arithmetic contract: compiled with -ffp-contract=off, every + - * / below is ONE IEEE
// operation in the order written, so results are bit-identical to a scalar CPU evaluation
// of the same expressions (the parity tests rely on this).  Operation order follows the
// reference scripts; each operator cites the lines it restates.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "lbm_rheology.hpp"   // the rheology table's index, host and device (lbm_set_rheology)

namespace lbm {

constexpr int Q = 9;
constexpr int GH = 4;  // ghost/pad columns on each side of a row (keeps x = 0 16-byte aligned)
constexpr int GHY = 10; // ghost rows above and below a lattice: row -1 / ny is the one-row halo of a slab (and holds parked wall data);
                        // rows -S .. -1 / ny .. ny+S-1 receive the neighbour's rows for the multi-step launches (deep halo, S <= 8)

// a1: lattice vectors, MRT.py:138-140 (k: 0 rest, 1 E, 2 N, 3 W, 4 S, 5 NE, 6 NW, 7 SW, 8 SE).
// A population moves from (x, y) to (x + cx, y - cy): y = 0 is the lid (MRT_GPU.py:412-413).
__host__ __device__ constexpr int cxk(int k) { return k == 1 || k == 5 || k == 8 ? 1 : (k == 3 || k == 6 || k == 7 ? -1 : 0); }
__host__ __device__ constexpr int cyk(int k) { return k == 2 || k == 5 || k == 6 ? 1 : (k == 4 || k == 7 || k == 8 ? -1 : 0); }

enum { SEM_PY = 0, SEM_GPU = 1, SEM_BB = 2, SEM_SOLID = 3 };   // = lbm_params.semantics (LBM_SEM_MRT_PY, LBM_SEM_MRT_GPU, LBM_SEM_BOUNCE_BACK, LBM_SEM_BOUNCE_BACK_SOLID)
// SEM_SOLID is SEM_BB plus solid cells: everything that asks "bounce-back walls?" asks sem_is_bb
constexpr bool sem_is_bb(int sem) { return sem == SEM_BB || sem == SEM_SOLID; }
enum { C_SRT = 0, C_TRT = 1, C_MRT = 2,
       // lbm_params.arith = LBM_ARITH_FAST: not the reference's operation order / rounding --
       C_MRT_FAST = 3,     // the MRT operator in factored form with fused multiply-adds
       C_SRT_FAST = 4,     // SRT / TRT as in the strict form, but u = j * rcp(rho) and the closure's divisions and square root by
       C_TRT_FAST = 5,     // v_rcp_f32 / v_sqrt_f32 (1 ulp; fp64: v_rcp_f64 / v_rsq_f64 + Newton) instead of the IEEE sequences
       // lbm_params.arith = LBM_ARITH_PROMOTED (fp32 only): the strict operators, but the sub-expressions that MRT_GPU.py's CUDA text
       // evaluates in double -- its double literals in float expressions, C's usual arithmetic conversions (MRT_GPU.py:385, 410,
       // 638-642, 652) -- are evaluated in double and rounded to float once, as the CPU oracles' promote = True
       C_SRT_PROM = 6, C_TRT_PROM = 7, C_MRT_PROM = 8 };
constexpr bool coll_is_mrt(int c) { return c == C_MRT || c == C_MRT_FAST || c == C_MRT_PROM; }
constexpr bool coll_is_fast(int c) { return c == C_MRT_FAST || c == C_SRT_FAST || c == C_TRT_FAST; }
constexpr bool coll_is_prom(int c) { return c == C_SRT_PROM || c == C_TRT_PROM || c == C_MRT_PROM; }

template <typename R>
struct Relax {  // a2: MRT_GPU.py:63-93
    R uLB, w_nu, w_m, w_e, w_eps, w_q;
};

// The operators below are written once for a value type T that is either a scalar real or a 2-wide extended vector of
// reals (two cells side by side): on gfx950 fp32 pairs compile to packed v_pk_add_f32 / v_pk_mul_f32, lane-wise IEEE, so the
// results are the same bits as the scalar evaluation.  S = ScalarOf<T>::type is the type of the constants.
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <typename T> struct ScalarOf { typedef T type; };
template <> struct ScalarOf<f32x2> { typedef float type; };

// Destination window of direction k (a7).  SEM_PY: the truncated slices of MRT.py:404-414;
// SEM_GPU: "neighbour inside the lattice", MRT_GPU.py:412.  SEM_BB: every slot of every cell streams (a source outside the
// lattice is the bounce-back of gather_a, not a kept slot).  gy is the GLOBAL row.
template <int SEM>
__device__ __forceinline__ bool in_window(int k, int x, int gy, int X, int Y) {
    const int cx = cxk(k), cy = cyk(k);
    bool ok = true;
    if (sem_is_bb(SEM)) {
        return true;
    } else if (SEM == SEM_PY) {
        if (cx > 0) ok = ok && (x >= 1) && (x <= X - 2);
        if (cx < 0) ok = ok && (x <= X - 3);
        if (cy > 0) ok = ok && (gy <= Y - 3);
        if (cy < 0) ok = ok && (gy >= 1) && (gy <= Y - 2);
    } else {
        if (cx > 0) ok = ok && (x >= 1);
        if (cx < 0) ok = ok && (x <= X - 2);
        if (cy > 0) ok = ok && (gy <= Y - 2);
        if (cy < 0) ok = ok && (gy >= 1);
    }
    return ok;
}

// a3: equilibrium, MRT.py:213-231 / MRT_GPU.py:408-410.  cu is formed without the
// multiplications by 0 and +-1 of the reference (value-identical in IEEE arithmetic).
template <typename T>
__device__ __forceinline__ T cu_of(int k, T ux, T uy) {
    switch (k) {
        case 1: return ux;
        case 2: return uy;
        case 3: return -ux;
        case 4: return -uy;
        case 5: return ux + uy;
        case 6: return -ux + uy;
        case 7: return -ux + -uy;
        case 8: return ux + -uy;
        default: return T{};
    }
}
template <typename R>
__device__ __forceinline__ R weight(int k) {
    return k == 0 ? (R)(4.0 / 9.0) : (k < 5 ? (R)(1.0 / 9.0) : (R)(1.0 / 36.));
}
// a / b and sqrt: IEEE-exact, or (FAST, fp32 only) by v_rcp_f32 / v_sqrt_f32 (1 ulp) -- the same instruction per lane in the
// scalar and the packed form, so every kernel variant still produces the same bits
template <bool FAST> __device__ __forceinline__ float div_(float a, float b) { return FAST ? a * __builtin_amdgcn_rcpf(b) : a / b; }
// fp64: v_rcp_f64 / v_rsq_f64 (about 2^-26) refined by two Newton steps (error far below one ulp of the iterate; the product with
// `a` rounds once more) instead of the IEEE sequences of ~25 instructions
__device__ __forceinline__ double rcp_nr(double b) {
    double r = __builtin_amdgcn_rcp(b);
    r = __builtin_fma(__builtin_fma(-b, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-b, r, 1.0), r, r);
    return r;
}
template <bool FAST> __device__ __forceinline__ double div_(double a, double b) { return FAST ? a * rcp_nr(b) : a / b; }
template <bool FAST> __device__ __forceinline__ f32x2 div_(f32x2 a, f32x2 b) {
    return FAST ? a * f32x2{__builtin_amdgcn_rcpf(b.x), __builtin_amdgcn_rcpf(b.y)} : a / b;
}
template <bool FAST> __device__ __forceinline__ float sqrt_(float a) { return FAST ? __builtin_amdgcn_sqrtf(a) : sqrtf(a); }
template <bool FAST> __device__ __forceinline__ double sqrt_(double a) {
    if (!FAST) return sqrt(a);
    if (a <= 0.0) return 0.0;                        // (the closure's argument is tau0^2 + ... > 0)
    double y = __builtin_amdgcn_rsq(a);              // 1 / sqrt(a), ~2^-26
    y = y * __builtin_fma(-0.5 * a * y, y, 1.5);     // Newton on 1 / sqrt
    y = y * __builtin_fma(-0.5 * a * y, y, 1.5);
    const double g = a * y;                          // sqrt(a), then one correction step
    return __builtin_fma(__builtin_fma(-g, g, a), 0.5 * y, g);
}
template <bool FAST> __device__ __forceinline__ f32x2 sqrt_(f32x2 a) {
    return FAST ? f32x2{__builtin_amdgcn_sqrtf(a.x), __builtin_amdgcn_sqrtf(a.y)} : f32x2{sqrtf(a.x), sqrtf(a.y)};
}

// Promoted arithmetic works on one fp32 value at a time (packed math has no double lanes): f applied to each lane of f32x2 arguments
template <typename F> __device__ __forceinline__ float lanes(F f, float a, float b) { return f(a, b); }
template <typename F> __device__ __forceinline__ f32x2 lanes(F f, f32x2 a, f32x2 b) { return f32x2{f(a.x, b.x), f(a.y, b.y)}; }
template <typename F> __device__ __forceinline__ float lanes(F f, float a, float b, float c) { return f(a, b, c); }
template <typename F> __device__ __forceinline__ f32x2 lanes(F f, f32x2 a, f32x2 b, f32x2 c) { return f32x2{f(a.x, b.x, c.x), f(a.y, b.y, c.y)}; }

// promoted equilibrium (MRT_GPU.py:410,652 `rho_l*t_g[k]*(1. + 3.0*cu + 9*0.5*cu*cu - 3.0*0.5*usqr)`): rt = rho t_k
// is float * float, the bracket and its product with rt are double, one rounding at the store
__device__ __forceinline__ float feq_prom(float rt, float cu, float usqr) {
    const double c = (double)cu;
    return (float)((double)rt * (((1. + 3.0 * c) + (4.5 * c) * c) - 1.5 * (double)usqr));
}
__device__ __forceinline__ f32x2 feq_prom(f32x2 rt, f32x2 cu, f32x2 usqr) {
    return f32x2{feq_prom(rt.x, cu.x, usqr.x), feq_prom(rt.y, cu.y, usqr.y)};
}

// PROM (fp32 only): the promoted form above
template <typename T, bool PROM = false>
__device__ __forceinline__ void equ(T rho, T ux, T uy, T (&feq)[Q]) {
    typedef typename ScalarOf<T>::type S;
    const T usqr = ux * ux + uy * uy;
    if constexpr (PROM) {
#pragma unroll
        for (int k = 0; k < Q; ++k) feq[k] = feq_prom(rho * weight<S>(k), cu_of<T>(k, ux, uy), usqr);
        return;
    }
    const T c = (S)1.5 * usqr;
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        const T cu = cu_of<T>(k, ux, uy);
        feq[k] = (rho * weight<S>(k)) * ((((S)1. + (S)3.0 * cu) + ((S)4.5 * cu) * cu) - c);
    }
}

// a4 + a5: moments with the macroscopic wall overrides (MRT.py:292,320-321,337,341-342;
// MRT_GPU.py:389-405).  SEM_BB: the plain moments on every cell (all of them are fluid cells; no override).
template <typename R, bool FAST = false, int SEM = SEM_GPU>
__device__ __forceinline__ void macros(const R (&f)[Q], int x, int gy, int X, int Y, R uLB, R& rho, R& ux, R& uy) {
    rho = ((((((((f[0] + f[1]) + f[2]) + f[3]) + f[4]) + f[5]) + f[6]) + f[7]) + f[8]);
    ux = div_<FAST>((((((f[1] - f[3]) + f[5]) - f[6]) - f[7]) + f[8]), rho);
    uy = div_<FAST>((((((f[2] - f[4]) + f[5]) + f[6]) - f[7]) - f[8]), rho);
    if (sem_is_bb(SEM)) return;   // (a solid cell of SEM_SOLID holds w_k: the sums give rho = sum w_k and u = exactly 0)
    if (x == 0 || x == X - 1 || gy == Y - 1) { ux = (R)0; uy = (R)0; }
    if (gy == 0) {
        rho = ((f[0] + f[1]) + f[3]) + (R)2. * ((f[2] + f[5]) + f[6]);
        ux = uLB; uy = (R)0;
    }
}

// fused multiply-add on a scalar real or on two packed cells (v_fma_f32 / v_fma_f64 / v_pk_fma_f32): one rounding, lane-wise
__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ f32x2 fma_(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

// a6: collision.  SRT MRT.py:396 / MRT_GPU.py:413; TRT MRT_GPU.py:455-462,514-525;
// MRT MRT_GPU.py:633-655 (m = M f with jx = m3, jy = m5 from the raw populations, the
// reference's own m_eq polynomial, f* = Minv m).  Zero matrix entries are skipped and the
// +-1, +-2, +-4 entries of M are exact scalings: value-identical to the dense products.
template <typename T, int COLL, bool WM = false>
__device__ __forceinline__ void collide(const T (&f)[Q], T rho, const T (&feq)[Q],
                                        const Relax<typename ScalarOf<T>::type>& w, T w_nu, T (&out)[Q], bool lid = false, T w_m = T{}) {
    // w_nu: the viscous rate of each cell (w.w_nu, the Smagorinsky value, or the cell's of a relaxation field); the other rates are
    // lattice-wide scalars -- but for WM (lbm_set_relaxation_field): TRT's odd rate of each cell is w_m, in the place of w.w_m
    // lid (C_MRT_FAST only): the cells are on the lid row, where rho is the overridden rho_l, not the population sum m0
    typedef typename ScalarOf<T>::type R;
    if (COLL == C_SRT || COLL == C_SRT_FAST || COLL == C_SRT_PROM) {
#pragma unroll
        for (int k = 0; k < Q; ++k) out[k] = f[k] - w_nu * (f[k] - feq[k]);
    } else if (COLL == C_TRT || COLL == C_TRT_FAST || COLL == C_TRT_PROM) {
        T fp[Q], fm[Q], ep[Q], em[Q];
        constexpr int pa[4] = {2, 5, 6, 1}, pb[4] = {4, 7, 8, 3};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int a = pa[i], b = pb[i];
            fp[a] = (R)0.5 * (f[a] + f[b]); fp[b] = fp[a];
            fm[a] = (R)0.5 * (f[a] - f[b]); fm[b] = -fm[a];
            ep[a] = (R)0.5 * (feq[a] + feq[b]); ep[b] = ep[a];
            em[a] = (R)0.5 * (feq[a] - feq[b]); em[b] = -em[a];
        }
        fp[0] = f[0]; fm[0] = T{}; ep[0] = feq[0]; em[0] = T{};
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            if constexpr (WM) out[k] = (f[k] - w_nu * (fp[k] - ep[k])) - w_m * (fm[k] - em[k]);
            else out[k] = (f[k] - w_nu * (fp[k] - ep[k])) - w.w_m * (fm[k] - em[k]);
        }
    } else if (COLL == C_MRT_FAST) {
        // The same operator, m = M f, m* = m - S (m - m_eq), f* = Minv m*, with the sums of M and Minv factored through the
        // pairs f1 +- f3, f2 +- f4, f5 +- f7, f6 +- f8 and explicit fused multiply-adds: ~75 operations per cell instead of
        // ~190.  Algebraically identical to the branch below, NOT the reference's operation order: results differ from the
        // strict form in the last bits (tests/test_arith_error_budget_gpu.py bounds the difference against a long-double reference;
        // tests/test_arith_error_budget_cpu.py checks the algebra).  The operations are spelled out (no compiler contraction), so
        // every kernel variant performs the same ones and a lattice gives the same bits however it is cut into tiles, frames or slabs.
        // m_eq[1], m_eq[2] take the density the strict form takes: rho, which is m0 everywhere but on the lid row (rho_l = f0 + f1
        // + f3 + 2 (f2 + f5 + f6), MRT_GPU.py:400-405,638-642).  m0 itself relaxes at rate 0 and goes into the back transform as r.
        // Off the lid the factored sum r stands in for rho (same number up to rounding), so the interior's operations are those of
        // the sum already formed; `lid` is a compile-time false in every kernel that never holds a lid cell.
        const T a13 = f[1] + f[3], d13 = f[1] - f[3], a24 = f[2] + f[4], d24 = f[2] - f[4];
        const T a57 = f[5] + f[7], d57 = f[5] - f[7], a68 = f[6] + f[8], d68 = f[6] - f[8];
        const T sa = a13 + a24, sd = a57 + a68, dm = d57 - d68, dp = d57 + d68;
        const T r = (f[0] + sa) + sd;                                       // m0
        const T jx = d13 + dm, jy = d24 + dp;                               // m3, m5
        const T f04 = (R)4 * f[0];
        T e = fma_(T((R)2), sd, -sa) - f04;                                 // m1
        T eps = fma_(T((R)-2), sa, f04 + sd);                               // m2
        T qx = fma_(T((R)-2), d13, dm), qy = fma_(T((R)-2), d24, dp);       // m4, m6
        T pxx = a13 - a24, pxy = a57 - a68;                                 // m7, m8
        const T jx2 = jx * jx, jy2 = jy * jy, j23 = (R)3 * (jx2 + jy2);
        const T rq = lid ? rho : r;                                         // the density of m_eq[1], m_eq[2]
        e = fma_(T(-w.w_e), e - fma_(T((R)-2), rq, j23), e);
        eps = fma_(T(-w.w_eps), eps - fma_(T((R)9), jx2 * jy2, rq - j23), eps);
        qx = fma_(T(-w.w_q), qx - jx * fma_(T((R)3), jx2, T((R)-1)), qx);
        qy = fma_(T(-w.w_q), qy - jy * fma_(T((R)3), jy2, T((R)-1)), qy);
        pxx = fma_(-w_nu, pxx - (jx2 - jy2), pxx);
        pxy = fma_(-w_nu, fma_(-jx, jy, pxy), pxy);
        const R a9 = (R)(1.0 / 9), a36 = (R)(1.0 / 36), a18 = (R)(1.0 / 18), a6 = (R)(1.0 / 6),
                a12 = (R)(1.0 / 12), a4 = (R)(1.0 / 4);
        const T r9 = a9 * r;
        out[0] = a9 * ((r - e) + eps);
        const T A = fma_(T(-a18), eps, fma_(T(-a36), e, r9)), D = fma_(T(a36), eps, fma_(T(a18), e, r9));
        const T Ap = fma_(T(a4), pxx, A), Am = fma_(T(-a4), pxx, A), Dp = fma_(T(a4), pxy, D), Dm = fma_(T(-a4), pxy, D);
        const T bx = a6 * (jx - qx), by = a6 * (jy - qy);
        const T X = fma_(T(a12), qx, a6 * jx), Y = fma_(T(a12), qy, a6 * jy);
        const T XpY = X + Y, XmY = X - Y;
        out[1] = Ap + bx; out[3] = Ap - bx;
        out[2] = Am + by; out[4] = Am - by;
        out[5] = Dp + XpY; out[7] = Dp - XpY;
        out[8] = Dm + XmY; out[6] = Dm - XmY;
    } else {
        T m[Q], meq[Q];
        // rows of M_GS (MRT.py:163-173), left-to-right sums.  A term  acc + c * x  with c = +-2, +-4 or +-1/4 is written as ONE fused
        // multiply-add: the product by a power of two is exact, so round(acc + c x) is the same number whether the product is
        // rounded first (the reference: multiply, then add) or not -- same bits, one instruction instead of two (19 of ~160
        // operations per cell; 4096^2 strict: fp32 247 -> 270 GLUPS, fp64 118 -> 125, every test still bit-identical to the oracle).  Products by 3, 9, 1/9 ... are not exact and stay two operations.
        const T c2 = T((R)2), cm2 = T((R)-2);
        m[0] = (((((((f[0] + f[1]) + f[2]) + f[3]) + f[4]) + f[5]) + f[6]) + f[7]) + f[8];
        m[1] = fma_(c2, f[8], fma_(c2, f[7], fma_(c2, f[6], fma_(c2, f[5], ((((R)-4 * f[0] - f[1]) - f[2]) - f[3]) - f[4]))));
        m[2] = (((fma_(cm2, f[4], fma_(cm2, f[3], fma_(cm2, f[2], fma_(cm2, f[1], (R)4 * f[0])))) + f[5]) + f[6]) + f[7]) + f[8];
        m[3] = ((((f[1] - f[3]) + f[5]) - f[6]) - f[7]) + f[8];
        m[4] = (((fma_(c2, f[3], (R)-2 * f[1]) + f[5]) - f[6]) - f[7]) + f[8];
        m[5] = ((((f[2] - f[4]) + f[5]) + f[6]) - f[7]) - f[8];
        m[6] = (((fma_(c2, f[4], (R)-2 * f[2]) + f[5]) + f[6]) - f[7]) - f[8];
        m[7] = ((f[1] - f[2]) + f[3]) - f[4];
        m[8] = ((f[5] - f[6]) + f[7]) - f[8];
        const T jx = m[3], jy = m[5];
        meq[0] = rho;
        meq[1] = fma_(cm2, rho, (R)3.0 * (jx * jx + jy * jy));
        meq[2] = ((R)-3.0 * (jx * jx + jy * jy) + rho) + (R)9.0 * (((jx * jx) * jy) * jy);
        meq[3] = m[3];
        meq[4] = -jx + (R)3.0 * ((jx * jx) * jx);
        meq[5] = m[5];
        meq[6] = -jy + (R)3.0 * ((jy * jy) * jy);
        meq[7] = jx * jx - jy * jy;
        meq[8] = jx * jy;
        if constexpr (COLL == C_MRT_PROM) {
            // MRT_GPU.py:638-642: the literals -2.0, 3.0, 9.0 make these four sums double, one rounding each;
            // the products of jx, jy among themselves stay float (and the strict form's multiply-add for meq[1] is not used here)
            const T s = jx * jx + jy * jy, p4 = ((jx * jx) * jy) * jy, x3 = (jx * jx) * jx, y3 = (jy * jy) * jy;
            meq[1] = lanes([](float r, float a) { return (float)(-2.0 * (double)r + 3.0 * (double)a); }, rho, s);
            meq[2] = lanes([](float a, float r, float b) { return (float)((-3.0 * (double)a + (double)r) + 9.0 * (double)b); }, s, rho, p4);
            meq[4] = lanes([](float j, float a) { return (float)((double)(-j) + 3.0 * (double)a); }, jx, x3);
            meq[6] = lanes([](float j, float a) { return (float)((double)(-j) + 3.0 * (double)a); }, jy, y3);
        }
        // The reference relaxes all nine moments, three of them with rate 0 (MRT.py:141, MRT_GPU.py:650: m[k] - 0 * (m[k] - meq[k]) for the
        // density and the two momenta).  That is m[k] itself, bit for bit, for every finite input: 0 * x = +-0 and m - (+-0) = m unless m is
        // a zero of the other sign -- and there meq[k] = m[k] (k = 3, 5: x - x = +0, so the product is +0 and -0 - (+0) = -0 stays), while
        // m[0] is a positive density.  Left out: nine operations of ~150 per cell (4096^2 strict fp32 302 -> 307 GLUPS, fp64 136 -> 141), every strict test still
        // np.array_equal to the oracle, which spells the three out.
        m[1] = m[1] - w.w_e * (m[1] - meq[1]);
        m[2] = m[2] - w.w_eps * (m[2] - meq[2]);
        m[4] = m[4] - w.w_q * (m[4] - meq[4]);
        m[6] = m[6] - w.w_q * (m[6] - meq[6]);
        m[7] = m[7] - w_nu * (m[7] - meq[7]);
        m[8] = m[8] - w_nu * (m[8] - meq[8]);
        // rows of M_GS_INV (MRT.py:175-183)
        const R a9 = (R)(1.0 / 9), a36 = (R)(1.0 / 36), a18 = (R)(1.0 / 18), a6 = (R)(1.0 / 6),
                a12 = (R)(1.0 / 12), a4 = (R)(1.0 / 4);
        const T q4 = T(a4), qm4 = T(-a4);
        out[0] = (a9 * m[0] + -a9 * m[1]) + a9 * m[2];
        out[1] = fma_(q4, m[7], (((a9 * m[0] + -a36 * m[1]) + -a18 * m[2]) + a6 * m[3]) + -a6 * m[4]);
        out[2] = fma_(qm4, m[7], (((a9 * m[0] + -a36 * m[1]) + -a18 * m[2]) + a6 * m[5]) + -a6 * m[6]);
        out[3] = fma_(q4, m[7], (((a9 * m[0] + -a36 * m[1]) + -a18 * m[2]) + -a6 * m[3]) + a6 * m[4]);
        out[4] = fma_(qm4, m[7], (((a9 * m[0] + -a36 * m[1]) + -a18 * m[2]) + -a6 * m[5]) + a6 * m[6]);
        out[5] = fma_(q4, m[8], (((((a9 * m[0] + a18 * m[1]) + a36 * m[2]) + a6 * m[3]) + a12 * m[4]) + a6 * m[5]) + a12 * m[6]);
        out[6] = fma_(qm4, m[8], (((((a9 * m[0] + a18 * m[1]) + a36 * m[2]) + -a6 * m[3]) + -a12 * m[4]) + a6 * m[5]) + a12 * m[6]);
        out[7] = fma_(q4, m[8], (((((a9 * m[0] + a18 * m[1]) + a36 * m[2]) + -a6 * m[3]) + -a12 * m[4]) + -a6 * m[5]) + -a12 * m[6]);
        out[8] = fma_(qm4, m[8], (((((a9 * m[0] + a18 * m[1]) + a36 * m[2]) + a6 * m[3]) + a12 * m[4]) + -a6 * m[5]) + -a12 * m[6]);
    }
}

// Smagorinsky sub-grid closure, MRT_GPU.py:368-387 (turb = 1).  The Van Driest lines 370-373 are
// dead code (Cs2 is overwritten by 0.025 at line 374).  The reference reads, per cell, the
// equilibrium and the density that funRT wrote in the PREVIOUS step; only sum_k cx cy feq_k of it
// is used, so the history kept per cell is two reals: planes Q (that sum) and Q + 1 (density).
constexpr int K_QEQ = Q;      // plane index of  -feq8 + (feq7 + (-feq6 + feq5))  of the previous step
constexpr int K_RHO = Q + 1;  // plane index of the previous step's density (after the lid override)

template <typename T>
__device__ __forceinline__ T diag_flux(const T (&f)[Q]) {   // product = cx cy f_k + product, k = 0..8
    return -f[8] + (f[7] + (-f[6] + f[5]));
}
// Equilibrium + collision of a cell (or of two packed cells) from its macroscopic state, as every step kernel calls it; q2 (TURB only):
// sum_k cx cy feq_k of THIS step, the closure's history (K_QEQ).  The strict operators and the factored MRT one: equ() -> collide() ->
// diag_flux(), exactly the sequence the kernels spelled out before.  C_SRT_FAST / C_TRT_FAST (r03): the same operators with the
// equilibrium never formed -- feq_k = rho t_k (B + 4.5 cu^2 +- 3 cu), B = 1 - 1.5 u^2, shares everything but the sign of the odd part
// between the two directions of a pair, so
//   SRT  f*_k = (1 - w) f_k + (w rho t_k) (E_k +- O_k),                      E = B + 4.5 cu^2, O = 3 cu
//   TRT  f*_a/b = f_a/b - P -+ M,  P = w+ ((f_a + f_b) / 2 - rho t E),  M = w- ((f_a - f_b) / 2 - rho t O)
// with fused multiply-adds: ~50 / ~65 operations per cell after the moments instead of ~105 / ~140, and sum_k cx cy feq_k = rho ux uy
// exactly.  Same operator, other rounding: NOT the reference's operation order (tolerances: tests/test_gpu_parity.py::test_fast_arithmetic_*);
// one spelling for every kernel, so a lattice gives the same bits however it is cut.
// WM (the kernels of a relaxation field alone, lbm_set_relaxation_field): w_m is TRT's odd rate of each cell, in the place of w.w_m -- the
// same operations on a value per cell.
template <typename T, int COLL, bool TURB, bool WM = false>
__device__ __forceinline__ void equ_collide(const T (&g)[Q], T rho, T ux, T uy, const Relax<typename ScalarOf<T>::type>& w, T w_nu, T (&out)[Q], T& q2,
                                            bool lid = false, T w_m = T{}) {   // lid: the cells are on the lid row (only the factored MRT form asks)
    typedef typename ScalarOf<T>::type R;
    // (fp32 SRT with the closure keeps the unfused sequence: at the streaming kernels' 128 registers the fused one spills there -- 4096^2
    // 256 -> 210 GLUPS, while fp64 gains, 108 -> 134; without the closure it is what lets fp32 SRT take the walls kernel, 251 -> 414)
    if constexpr ((COLL == C_SRT_FAST && !(TURB && sizeof(R) == 4)) || COLL == C_TRT_FAST) {
        const T base = fma_(T((R)-1.5), fma_(uy, uy, ux * ux), T((R)1));
        const T orho = w_nu * rho, c1 = (R)1 - w_nu;
        const T r1 = (R)(1.0 / 9) * orho, r5 = (R)(1.0 / 36) * orho;
        out[0] = fma_((R)(4.0 / 9) * orho, base, c1 * g[0]);
        if constexpr (COLL == C_SRT_FAST) {
            auto pair = [&](T cu, T rw, const T& ga, const T& gb, T& oa, T& ob) {
                const T e = fma_((R)4.5 * cu, cu, base), o = (R)3 * cu;
                oa = fma_(rw, e + o, c1 * ga);
                ob = fma_(rw, e - o, c1 * gb);
            };
            pair(ux, r1, g[1], g[3], out[1], out[3]);
            pair(uy, r1, g[2], g[4], out[2], out[4]);
            pair(ux + uy, r5, g[5], g[7], out[5], out[7]);
            pair(ux - uy, r5, g[8], g[6], out[8], out[6]);
        } else {
            const auto wm = [&] { if constexpr (WM) return w_m; else return w.w_m; }();   // (T per cell, or the lattice's R)
            const T mrho = wm * rho, hp = (R)0.5 * w_nu;
            const T m1 = (R)(1.0 / 9) * mrho, m5 = (R)(1.0 / 36) * mrho;
            const auto hm = (R)0.5 * wm;
            auto pair = [&](T cu, T rp, T rm, const T& ga, const T& gb, T& oa, T& ob) {
                const T e = fma_((R)4.5 * cu, cu, base), o = (R)3 * cu;
                const T P = fma_(-rp, e, hp * (ga + gb)), M = fma_(-rm, o, hm * (ga - gb));
                oa = (ga - P) - M;
                ob = (gb - P) + M;
            };
            pair(ux, r1, m1, g[1], g[3], out[1], out[3]);
            pair(uy, r1, m1, g[2], g[4], out[2], out[4]);
            pair(ux + uy, r5, m5, g[5], g[7], out[5], out[7]);
            pair(ux - uy, r5, m5, g[8], g[6], out[8], out[6]);
        }
        if (TURB) q2 = rho * (ux * uy);
    } else if constexpr (COLL == C_MRT_FAST) {
        // (the MRT operator needs neither u nor feq, MRT_GPU.py:633-648; the closure's history sum_k cx cy feq_k is rho ux uy, see above --
        // the nine equilibria the strict form builds for it are left out: 4096^2 MRT + closure fp32 212 -> 283 GLUPS, fp64 91 -> 117)
        T fe[Q];
        collide<T, COLL>(g, rho, fe, w, w_nu, out, lid);
        if (TURB) q2 = rho * (ux * uy);
    } else {
        T fe[Q];
        if (!coll_is_mrt(COLL) || TURB) equ<T, coll_is_prom(COLL)>(rho, ux, uy, fe);     // (the plain MRT operator needs neither u nor feq: MRT_GPU.py:633-648)
        if constexpr (WM) collide<T, COLL, true>(g, rho, fe, w, w_nu, out, false, w_m);
        else collide<T, COLL>(g, rho, fe, w, w_nu, out);
        if (TURB) q2 = diag_flux<T>(fe);
    }
}

__device__ __forceinline__ float real_abs(float x) { return fabsf(x); }
__device__ __forceinline__ double real_abs(double x) { return fabs(x); }
__device__ __forceinline__ f32x2 real_abs(f32x2 x) { return f32x2{fabsf(x.x), fabsf(x.y)}; }

// T: scalar real or f32x2; the result is the per-cell relaxation rate (a T, not a scalar)
template <typename T, bool FAST = false, bool PROM = false>
__device__ __forceinline__ T smagorinsky_tau(const T (&f)[Q], T qeq_prev, T rho_prev, typename ScalarOf<T>::type omega) {   // taus_g, MRT_GPU.py:385-387
    typedef typename ScalarOf<T>::type R;
    const R tau0 = (R)1.0 / omega;
    const T q = diag_flux<T>(f) - qeq_prev;
    if constexpr (PROM) {
        // MRT_GPU.py:385: tau*tau is float * float, Cs2 the float 0.025f, abs(float) float; the rest is double
        // (18*1.4142 is a double constant) -- IEEE double square root and division -- and rounded to float once
        const R tt = tau0 * tau0;
        return lanes([tau0, tt](float qq, float rp) {
            return (float)(0.5 * ((double)tau0 + sqrt((double)tt + (((18 * 1.4142) * (double)0.025f) * (double)fabsf(qq)) / (double)rp)));
        }, q, rho_prev);
    }
    return (R)0.5 * (tau0 + sqrt_<FAST>(tau0 * tau0 + div_<FAST>(((R)(18 * 1.4142) * (R)0.025) * real_abs(q), rho_prev)));
}
template <typename T, bool FAST = false, bool PROM = false>
__device__ __forceinline__ T smagorinsky_omega(const T (&f)[Q], T qeq_prev, T rho_prev, typename ScalarOf<T>::type omega) {
    typedef typename ScalarOf<T>::type R;
    return div_<FAST>(T((R)1.0), smagorinsky_tau<T, FAST, PROM>(f, qeq_prev, rho_prev, omega));
}

// The local sub-grid closure of the obstacle lattices (lbm_set_subgrid; Hou et al. 1996; no reference counterpart: DESIGN.md 2.10).  From
// the gathered populations of a cell and the moments the collision takes anyway, the whole non-equilibrium momentum flux -- all three
// components, so the rule does not know the axes --
//     Sxx = ((((f1 + f3) + f5) + f6) + f7) + f8      Syy = ((((f2 + f4) + f5) + f6) + f7) + f8      Sxy = ((f5 - f6) + f7) - f8
//     Pxx = Sxx - (rho / 3 + (rho ux) ux)            Pyy = Syy - (rho / 3 + (rho uy) uy)            Pxy = Sxy - (rho ux) uy
//     N   = sqrt((Pxx Pxx + 2 (Pxy Pxy)) + Pyy Pyy)
//     tau = 0.5 (tau0 + sqrt(tau0 tau0 + (k N) / rho)),   tau0 = 1 / omega,   k = 18 sqrt(2) Cs2 (formed in double on the host, rounded once)
// every operation in the lattice type, one rounding each, in the order written (rho / 3 is rho * (R)(1.0 / 3)); FAST: the two square roots
// and the two divisions ((k N) / rho here, 1 / tau in subgrid_omega) by sqrt_<FAST> / div_<FAST>, as the closure above.  No history: the
// step that computes tau uses it.  tests/subgrid_ref.py restates the order.
// W: the type of omega -- the lattice's rate, a scalar, or (a relaxation field, lbm_set_relaxation_field) the cells' own, a T: tau0 is then
// 1 / omega of the cell, the same division per cell.
template <typename T, bool FAST = false, typename W = typename ScalarOf<T>::type>
__device__ __forceinline__ T subgrid_tau(const T (&f)[Q], T rho, T ux, T uy, W omega, typename ScalarOf<T>::type k) {
    typedef typename ScalarOf<T>::type R;
    const W tau0 = (R)1.0 / omega;
    const T sxx = ((((f[1] + f[3]) + f[5]) + f[6]) + f[7]) + f[8];
    const T syy = ((((f[2] + f[4]) + f[5]) + f[6]) + f[7]) + f[8];
    const T sxy = ((f[5] - f[6]) + f[7]) - f[8];
    const T r3 = rho * (R)(1.0 / 3), jx = rho * ux;
    const T pxx = sxx - (r3 + jx * ux);
    const T pyy = syy - (r3 + (rho * uy) * uy);
    const T pxy = sxy - jx * uy;
    const T n = sqrt_<FAST>((pxx * pxx + (R)2 * (pxy * pxy)) + pyy * pyy);
    return (R)0.5 * (tau0 + sqrt_<FAST>(tau0 * tau0 + div_<FAST>(k * n, rho)));
}
template <typename T, bool FAST = false, typename W = typename ScalarOf<T>::type>
__device__ __forceinline__ T subgrid_omega(const T (&f)[Q], T rho, T ux, T uy, W omega, typename ScalarOf<T>::type k) {
    typedef typename ScalarOf<T>::type R;
    return div_<FAST>(T((R)1.0), subgrid_tau<T, FAST, W>(f, rho, ux, uy, omega, k));
}

// The rheology table of the obstacle lattices (lbm_set_rheology; a generalised Newtonian fluid): the viscous rate of a cell
// as a function of its own shear.  From the gathered populations and the moments the collision takes anyway, the DEVIATORIC part of the
// non-equilibrium momentum flux (MRT relaxes the trace at omega_e, so only the deviatoric moments belong to omega_nu; the rho / 3 cancels)
//     jx = rho ux                      jy = rho uy
//     a  = ((f1 + f3) - (f2 + f4)) - (jx ux - jy uy)          (= Pxx - Pyy)
//     b  = (((f5 - f6) + f7) - f8) - jx uy                    (= Pxy)
//     N  = sqrt(0.5 (a a) + 2 (b b))                          g = N / rho
//     s  = g inv_dg      i, fr = rheology_index(s)            w_nu = t[i] + fr d[i]     and, with a second table,  w_m = tm[i] + fr dm[i]
// every operation in the lattice type, one rounding each, in the order written, nothing fused.  FAST: the square root and the division by
// sqrt_<FAST> / div_<FAST>, and the interpolation is one fused multiply-add.  g needs no tau: the host has solved the implicit relation
// between the shear rate and tau once, when it tabulated omega over g.  No history and no store.  tests/rheology_ref.py restates the order.
// Rheo: the table (rheology_table of lbm_rheology.hpp, RHEO_STRIDE reals per entry), n - 1, inv_dg and whether the table carries TRT's odd
// rate; the context's, shared by every lattice of a batch.
template <typename R>
struct Rheo {
    const R* tab;
    R inv_dg;
    int nm1;
    int has_m;
};
struct RheoNone {};   // (what a kernel without a table passes in its place: nothing)
template <typename T, bool FAST = false>
__device__ __forceinline__ T rheology_shear(const T (&f)[Q], T rho, T ux, T uy) {
    typedef typename ScalarOf<T>::type R;
    const T jx = rho * ux, jy = rho * uy;
    const T a = ((f[1] + f[3]) - (f[2] + f[4])) - (jx * ux - jy * uy);
    const T b = (((f[5] - f[6]) + f[7]) - f[8]) - jx * uy;
    const T n = sqrt_<FAST>((R)0.5 * (a * a) + (R)2 * (b * b));
    return div_<FAST>(n, rho);
}
template <typename R, bool FAST>
__device__ __forceinline__ void rheology_lookup(R s, const Rheo<R>& rh, R w_m0, R& w_nu, R& w_m) {
    typedef R P __attribute__((ext_vector_type(2)));   // (a rate's value and slope: one 8- or 16-byte load)
    R fr;
    const int i = rheology_index<R>(s, rh.nm1, fr);
    const R* const e = rh.tab + (long long)i * RHEO_STRIDE;
    const P td = *reinterpret_cast<const P*>(e);
    w_nu = FAST ? fma_(fr, td.y, td.x) : td.x + fr * td.y;
    w_m = w_m0;
    if (rh.has_m) {   // (wave-uniform)
        const P md = *reinterpret_cast<const P*>(e + 2);
        w_m = FAST ? fma_(fr, md.y, md.x) : md.x + fr * md.y;
    }
}
// w_m0: the lattice's odd rate, what w_m is without a second table
template <typename T, bool FAST = false>
__device__ __forceinline__ void rheology_rates(const T (&f)[Q], T rho, T ux, T uy, const Rheo<typename ScalarOf<T>::type>& rh,
                                               typename ScalarOf<T>::type w_m0, T& w_nu, T& w_m) {
    const T s = rheology_shear<T, FAST>(f, rho, ux, uy) * rh.inv_dg;
    if constexpr (std::is_same<T, f32x2>::value) {   // (two cells side by side: a gather per half)
        float n0, m0, n1, m1;
        rheology_lookup<float, FAST>(s.x, rh, w_m0, n0, m0);
        rheology_lookup<float, FAST>(s.y, rh, w_m0, n1, m1);
        w_nu = f32x2{n0, n1};
        w_m = f32x2{m0, m1};
    } else {
        rheology_lookup<T, FAST>(s, rh, w_m0, w_nu, w_m);
    }
}

// a8: wall rules on the populations of ONE perimeter cell, given the equilibrium of the
// previous macroscopic state of that cell.  SEM_PY: MRT.py:450-453 in statement order
// (left equilibrium, right mirror pairing, bottom, lid); SEM_GPU: MRT_GPU.py:674-692
// (x rule if / else-if, then y rule if / else-if, opposite pairing).
template <typename R, int SEM>
__device__ __forceinline__ void wall_rules(R (&g)[Q], const R (&fe)[Q], int x, int gy, int X, int Y) {
    if (SEM == SEM_PY) {
        if (x == 0) { g[1] = fe[1]; g[5] = fe[5]; g[8] = fe[8]; }
        if (x == X - 1) {
            const R a = -fe[1] + (fe[3] + g[1]), b = -fe[5] + (fe[6] + g[5]), c = -fe[8] + (fe[7] + g[8]);
            g[3] = a; g[6] = b; g[7] = c;
        }
        if (gy == Y - 1) {
            const R a = -fe[4] + (fe[2] + g[4]), b = -fe[7] + (fe[5] + g[7]), c = -fe[8] + (fe[6] + g[8]);
            g[2] = a; g[5] = b; g[6] = c;
        }
        if (gy == 0) {
            const R a = -fe[2] + (fe[4] + g[2]), b = -fe[5] + (fe[7] + g[5]), c = -fe[6] + (fe[8] + g[6]);
            g[4] = a; g[7] = b; g[8] = c;
        }
    } else {
        if (x == 0) {
            g[1] = (fe[1] - fe[3]) + g[3];
            g[5] = (fe[5] - fe[7]) + g[7];
            g[8] = (fe[8] - fe[6]) + g[6];
        } else if (x == X - 1) {
            g[3] = (-fe[1] + fe[3]) + g[1];
            g[6] = (-fe[8] + fe[6]) + g[8];
            g[7] = (-fe[5] + fe[7]) + g[5];
        }
        if (gy == Y - 1) {
            g[2] = (-fe[4] + fe[2]) + g[4];
            g[5] = (-fe[7] + fe[5]) + g[7];
            g[6] = (-fe[8] + fe[6]) + g[8];
        } else if (gy == 0) {
            g[4] = (-fe[2] + fe[4]) + g[2];
            g[7] = (-fe[5] + fe[7]) + g[5];
            g[8] = (-fe[6] + fe[8]) + g[6];
        }
    }
}

// Addressing of the nine direction arrays.  Local row y in [-GHY, ny+GHY), column x in [-GH, nx+GH).
// Element (k, x, y) lives at k * plane + at(x, y).  Two layouts share this formula:
//   planes  [k][y][x]: plane = pitch * (ny + 2 GHY), row = pitch   (nine separate arrays)
//   rows    [y][k][x]: plane = pitch,            row = 9 * pitch   (the nine rows y of the nine
//                                                                   directions are adjacent)
// Every row of every direction is contiguous and 16-byte aligned in both.
struct Geo {
    long long plane;  // elements between the same cell of consecutive directions
    long long row;    // elements between consecutive rows of one direction
    int pitch;        // elements per row (nx + 2*GH, multiple of 4)
    int nx, ny;       // columns, local rows
    int y0, NY;       // first global row of this slab, global height
    __host__ __device__ __forceinline__ long long at(int x, int y) const { return (long long)(y + GHY) * row + GH + x; }
};

// The same (k, x, y) addressing for a small window of the lattice held in LDS (the fused frame passes keep the output of the
// intermediate passes there): window origin (x0, y0), `pitch` elements per row, `plane` per direction.  gather / update_cell
// take one addressing object for the source and one for the destination: Geo (a lattice in memory) or Window.
struct Window {
    int plane, pitch, x0, y0;
    __device__ __forceinline__ int at(int x, int y) const { return (y - y0) * pitch + (x - x0); }
};

// Where a perimeter cell parks the density of its last macroscopic state: slot 0 of the
// adjacent ghost cell (slot 0 of a ghost cell is never pulled).
template <typename A>
__device__ __forceinline__ auto wall_rho_at(const A& a, const Geo& g, int x, int y, int gy) -> decltype(a.at(x, y)) {
    if (gy == 0) return a.at(x, y - 1);
    if (gy == g.NY - 1) return a.at(x, y + 1);
    if (x == 0) return a.at(-1, y);
    return a.at(g.nx, y);
}

// Half-way bounce-back (SEM_BB): the opposite direction of k, and Ladd's moving-wall term of a slot whose source lies beyond the
// lid, 6 w_k rho_w (c_k . u_lid) with u_lid = (uLB, 0): +-t for the diagonals k = 8 / 7 (cx = +1 / -1), 0 for k = 4 (nothing is
// added there).  rho_w: the cell's parked density.  The one spelling of the term; tests/bounce_back_ref.py restates it.
__host__ __device__ constexpr int opp(int k) { return k == 0 ? 0 : (k < 5 ? (k + 1) % 4 + 1 : (k - 3) % 4 + 5); }
template <typename R>
__device__ __forceinline__ R lid_term(R rho_w, R uLB) { return (rho_w * uLB) * (R)(1.0 / 6.0); }

// Solid obstacles (SEM_SOLID): plane K_LINK of the lattice holds one small integer per cell, exact in fp32 and fp64 -- bit k - 1: the
// source (x - cx_k, y + cy_k) of slot k is a solid cell inside the lattice; bit 8: the cell itself is solid.  Written by lbm_set_solid
// into both lattices, never by a step.  A solid cell is never updated and holds the rest equilibrium w_k in both lattices.
// Bit 9: a hold cell (lbm_set_open_cells), whose word is exactly LINK_HOLD -- it is never updated either and holds its prescribed
// populations in both lattices, but it is no wall: a neighbour pulls from it by the plain pull, and no link bit points at it.
constexpr int K_LINK = Q;
constexpr int LINK_SOLID = 256;
constexpr int LINK_HOLD = 512;

// Curved obstacle surfaces (lbm_set_solid_shape; contract in include/lbm.h): the per-cell table of a shaped context, built on
// the host (lbm_wall_shape.hpp).  cell_row[ny][nx] of one lattice (x fastest): -1, or the cell's row; ad[rows][16] in the lattice type:
// slot k - 1 holds a, slot 8 + k - 1 holds d of the cell's link k; near[rows]: bit k - 1 set where link k interpolates with the next fluid
// cell.  Only cells with a link bit read it.
template <typename R>
struct ShapeTable {
    const int32_t* cell_row;
    const R* ad;
    const uint8_t* near;
};
// The interpolated bounce-back of one link, the one spelling every step kernel, gather and force kernel shares: own = the cell's
// post-collision population of direction opp(k); other = that of the next fluid cell (near) or the cell's own of direction k (far).
// Every operation in the lattice type, rounded in the order written.  a == 1 (the wall half-way) selects: no multiply by zero.
template <typename R>
__device__ __forceinline__ R shape_rule(R own, R other, R a, R d) {
    if (a == (R)1) return own + d;
    const R t1 = a * own, b = (R)1 - a, t2 = b * other;
    return (t1 + t2) + d;
}
// Link k of the cell at (x, y), from a lattice that holds post-collision populations and the cell's row of the table -- ad: its sixteen
// a and d, nm: its near bits, read by the caller.  The link's near bit picks `other`, the next fluid cell's population of direction
// opp(k) or the cell's own of direction k (far), one load from either place; a and d of the link go into shape_rule.  own: the cell's
// population of direction opp(k), which every caller holds already.  The force kernels call it; gather_a below and k_step_solid
// (lbm_solid.hpp) spell the same three lines in place, the one to keep the code of the reader kernels what it was, the
// other because both candidates for `other` are in registers there.
template <typename R, typename AS>
__device__ __forceinline__ R shape_link(const R* src, const AS& as, const R* ad, unsigned nm, int k, int x, int y, R own) {
    const bool near = (nm >> (k - 1)) & 1u;
    const R other = src[near ? opp(k) * as.plane + as.at(x + cxk(k), y - cyk(k)) : k * as.plane + as.at(x, y)];
    return shape_rule<R>(own, other, ad[k - 1], ad[8 + k - 1]);
}

// The mode of the obstacle wall rule, a compile-time argument of every kernel that applies it (the step kernels of lbm_solid.hpp,
// update_cell_a below, the force kernels of lbm_solid.hip and lbm_bodies.hip), and what the mode reads, the kernels' last argument;
// chosen on the host by with_wall_bits (lbm_host.hpp) alone.  A mode is base | bits: a base in the low two bits --
//   WALL_REST   every body at rest, no shape: the plain bounce, nothing to read
//   WALL_MOVE   a nonzero lbm_set_body_motion: a cell with links adds Ladd's term of link k to its post-collision population of
//               direction opp(k) before it stores it.  cell_row[batch][ny][nx] (x fastest; -1, or the cell's row of delta),
//               delta[rows][8] in the lattice type: lbm_wall_motion.hpp
//   WALL_SHAPE  lbm_set_solid_shape holds a shape: shape_rule on the read side of every link; the motion's term is part of the table, the
//               stores are the pure post-collision values
// -- and one bit per feature of the one-step kernels, each compile-time, so the kernels of a context without the feature are the
// instantiations they were, names and arguments included; update_cell_a and the force kernels take the base alone.
//   WALL_BUOY   buoyancy (lbm_set_buoyancy; Buoy below): by
//   WALL_SGS    the sub-grid closure (lbm_set_subgrid; subgrid_tau above): sgs = k = 18 sqrt(2) Cs2 in the lattice type.  Every cell that is
//               neither solid nor held takes w_nu = 1 / tau of its own gathered populations into the collision, in the place of the
//               lattice's rate; nothing else of the step changes
//   WALL_RELAX  a relaxation field (lbm_set_relaxation_field): rw, the plane of the cells' viscous rates (SRT's omega, TRT's omega+, MRT's
//               omega_nu), and rwm, the plane of TRT's omega- or null (every cell then keeps the lattice's w_m: a wave-uniform run-time
//               test) -- read-only, in the lattice type, addressed as the buoyancy plane (buoy_at; lattice z of a batch at
//               z * buoy_elems), so a vector's rates are one aligned 16-byte load.  Every cell that is neither solid nor held takes its
//               own rates into the collision; with the closure tau0 of subgrid_tau is 1 / rw of the cell
//   WALL_RHEO   a rheology table (lbm_set_rheology; rheology_rates above): rh.  Every cell that is neither solid nor held takes the rates
//               the table gives its own shear into the collision -- w_nu in the place of the lattice's rate and, where the table carries
//               it, TRT's odd rate; nothing else of the step changes
// Instantiated (lbm_solid.hpp) and picked (lbm_host.hpp): the three bases alone, with WALL_SGS, with WALL_RELAX and with both,
// WALL_BUOY on WALL_REST and WALL_MOVE alone -- the setters refuse buoyancy with a shape, the closure or a field -- and WALL_RHEO on the
// three bases alone: the table's setter and those of buoyancy, the closure and a field refuse each other.
constexpr int WALL_REST = 0, WALL_MOVE = 1, WALL_SHAPE = 2;
constexpr int WALL_BUOY = 4;
constexpr int WALL_SGS = 8;
constexpr int WALL_RELAX = 16;
constexpr int WALL_RHEO = 32;
constexpr int wall_base(int wall) { return wall & 3; }
constexpr bool wall_buoyant(int wall) { return (wall & WALL_BUOY) != 0; }
constexpr bool wall_subgrid(int wall) { return (wall & WALL_SGS) != 0; }
constexpr bool wall_relax(int wall) { return (wall & WALL_RELAX) != 0; }
constexpr bool wall_rheo(int wall) { return (wall & WALL_RHEO) != 0; }

// The uniform driving force (lbm_set_driving_force): f[k - 1] = F_k of direction k = 1 .. 8, rounded once to the lattice type on the host
// (drive_terms, lbm_periodic.hpp), and on != 0 while it is nonzero.  A kernel argument of the one-step obstacle kernels (lbm_solid.hpp);
// every cell that is neither solid nor held adds F_k to its post-collision population of direction k, one add in the lattice type, before
// the delta of WALL_MOVE.  Every other kernel passes the default, no force, and compiles to what it was.
template <typename R>
struct Drive {
    R f[8];
    int on;
};

// Buoyancy (lbm_set_buoyancy): the scalar acts on the flow.  cp: the buoyancy plane, one plane of the lattice's rows (buoy_at) that holds
// the C the most recent scalar step summed; b[k - 1] = B_k = (3 w_k)(cx_k ax + cy_k ay) in double (drive_terms) and c_ref, each rounded once
// to the lattice type on the host.  Every collision of a cell that is neither solid nor held is followed by
//     t = cp - c_ref;  d_k = F_k + B_k t;  fpost_k = fpost_k + d_k      (every operation in the lattice type, none fused)
// where the driving force is added alone without it.
// The plane has an addressing of its own, buoy_at: rows of geo.pitch elements with the lattice's ghost margins, whatever the lattice's
// layout is (in the rows layout Geo::at strides over all planes of a row and Geo::plane is one row).  buoy_at(x0, y) of a vector's first cell
// is 16-byte aligned where Geo::at(x0, y) is: pitch and Geo::row are multiples of 4.  buoy_elems: the elements of the allocation.
__host__ __device__ __forceinline__ long long buoy_at(const Geo& g, int x, int y) { return (long long)(y + GHY) * g.pitch + GH + x; }
__host__ __device__ __forceinline__ long long buoy_elems(const Geo& g) { return (long long)(g.ny + 2 * GHY) * g.pitch; }
template <typename R>
struct Buoy {
    const R* cp;
    R b[8];
    R c_ref;
};

// What a mode reads, composed of its parts in this order -- the base's tables, then each set bit's fields; a part is empty where the mode
// does not have it.
template <typename R, int BASE>
struct WallTables {};
template <typename R>
struct WallTables<R, WALL_MOVE> {
    const int32_t* cell_row;
    const R* delta;
};
template <typename R>
struct WallTables<R, WALL_SHAPE> {
    ShapeTable<R> sh;
};
template <typename R, bool ON>
struct WallBuoy {};
template <typename R>
struct WallBuoy<R, true> {
    Buoy<R> by;
};
template <typename R, bool ON>
struct WallSgs {};
template <typename R>
struct WallSgs<R, true> {
    R sgs;
};
template <typename R, bool ON>
struct WallField {};
template <typename R>
struct WallField<R, true> {
    const R* rw;
    const R* rwm;
};
template <typename R, bool ON>
struct WallRheo {};
template <typename R>
struct WallRheo<R, true> {
    Rheo<R> rh;
};
template <typename R, int WALL>
struct WallArg : WallTables<R, wall_base(WALL)>, WallBuoy<R, wall_buoyant(WALL)>, WallSgs<R, wall_subgrid(WALL)>, WallField<R, wall_relax(WALL)>,
                 WallRheo<R, wall_rheo(WALL)> {
    static constexpr int MODE = WALL;
};
// The kernel-argument layout of the modes in use: the sizes of the structs that spelled each mode's fields out in full
#define LBM_WALL_SIZE(WALL, F32, F64) static_assert(sizeof(WallArg<float, WALL>) == F32 && sizeof(WallArg<double, WALL>) == F64, "WallArg layout");
LBM_WALL_SIZE(WALL_REST, 1, 1) LBM_WALL_SIZE(WALL_MOVE, 16, 16) LBM_WALL_SIZE(WALL_SHAPE, 24, 24)
LBM_WALL_SIZE(WALL_REST | WALL_BUOY, 48, 80) LBM_WALL_SIZE(WALL_MOVE | WALL_BUOY, 64, 96)
LBM_WALL_SIZE(WALL_REST | WALL_SGS, 4, 8) LBM_WALL_SIZE(WALL_MOVE | WALL_SGS, 24, 24) LBM_WALL_SIZE(WALL_SHAPE | WALL_SGS, 32, 32)
LBM_WALL_SIZE(WALL_REST | WALL_RELAX, 16, 16) LBM_WALL_SIZE(WALL_MOVE | WALL_RELAX, 32, 32) LBM_WALL_SIZE(WALL_SHAPE | WALL_RELAX, 40, 40)
LBM_WALL_SIZE(WALL_REST | WALL_SGS | WALL_RELAX, 24, 24) LBM_WALL_SIZE(WALL_MOVE | WALL_SGS | WALL_RELAX, 40, 40)
LBM_WALL_SIZE(WALL_SHAPE | WALL_SGS | WALL_RELAX, 48, 48)
LBM_WALL_SIZE(WALL_REST | WALL_RHEO, 24, 24) LBM_WALL_SIZE(WALL_MOVE | WALL_RHEO, 40, 40) LBM_WALL_SIZE(WALL_SHAPE | WALL_RHEO, 48, 48)
#undef LBM_WALL_SIZE
// cell_row is [batch][ny][nx]: the offset of lattice z's table, and wa made the tables of that lattice -- the one spelling of the batch
// offset, whatever the mode (the vector kernel adds batch_cells to its own row offset, the other kernels call wall_batch)
__device__ __forceinline__ long long batch_cells(unsigned z, const Geo& geo) { return (long long)z * geo.nx * geo.ny; }
template <typename R, int WALL>
__device__ __forceinline__ void wall_batch(WallArg<R, WALL>& wa, unsigned z, const Geo& geo) {
    if constexpr (wall_base(WALL) == WALL_MOVE) wa.cell_row += batch_cells(z, geo);
    if constexpr (wall_base(WALL) == WALL_SHAPE) wa.sh.cell_row += batch_cells(z, geo);
}

// Gather the post-stream, post-wall-rule populations of cell (x, y) from a lattice that
// holds post-collision values (+ kept slots + parked wall densities); raw != 0: the lattice
// holds plain populations (state just set by the host), nothing to stream.  PROM: the wall rules' equilibrium in the promoted form.
// The link word of cell (x, y) as a gather from `src` sees it.  A lattice carries plane K_LINK itself; an LDS window (the fused frame
// passes) has no such plane -- no step writes it -- so there the word comes from `lnk`, plane K_LINK of the lattice the unit started from.
template <typename R, typename AS>
__device__ __forceinline__ int link_word(const R* __restrict__ src, const AS& as, const Geo& geo, const R* __restrict__ lnk, int x, int y) {
    if constexpr (std::is_same<AS, Window>::value) return (int)lnk[geo.at(x, y)];
    else return (int)src[K_LINK * as.plane + as.at(x, y)];
}

// SHAPE (SEM_SOLID on a lattice in memory, while lbm_set_solid_shape holds a shape; off everywhere else): a link takes shape_rule of the
// cell's table row instead of the plain bounce.
template <typename R, int SEM, typename AS, bool PROM = false, bool SHAPE = false>
__device__ __forceinline__ void gather_a(const R* __restrict__ src, const AS& as, const Geo& geo, int raw, R uLB, int x, int y, R (&g)[Q],
                                         const R* __restrict__ lnk = nullptr, ShapeTable<R> sh = ShapeTable<R>{}) {
    const int gy = geo.y0 + y;
    int lw = 0;
    if (SEM == SEM_SOLID) {
        lw = link_word<R, AS>(src, as, geo, lnk, x, y);
        if (lw & LINK_SOLID) {   // a solid cell: the constants it holds, whatever its neighbours stream
#pragma unroll
            for (int k = 0; k < Q; ++k) g[k] = weight<R>(k);
            return;
        }
    }
    if (raw || (SEM == SEM_SOLID && (lw & LINK_HOLD))) {   // (a hold cell: the nine values it holds, as every export sees them)
#pragma unroll
        for (int k = 0; k < Q; ++k) g[k] = src[k * as.plane + as.at(x, y)];
        return;
    }
#pragma unroll
    for (int k = 0; k < Q; ++k) g[k] = src[k * as.plane + as.at(x - cxk(k), y + cyk(k))];
    if (SEM == SEM_SOLID && (lw & 255)) {
        // a source inside the lattice that is a solid cell: the cell's own post-collision population of the opposite direction, nothing
        // added (obstacles are at rest).  Disjoint from the sources outside the lattice below.
#pragma unroll
        for (int k = 1; k < Q; ++k)
            if ((lw >> (k - 1)) & 1) g[k] = src[opp(k) * as.plane + as.at(x, y)];
        if constexpr (SHAPE) {
            // the plain bounce above is `own`; a near link's `other` is the regular pull of slot opp(k) (its source N is a fluid cell
            // inside the lattice), a far link's the cell's own stored slot k: one load from either place
            const int row = sh.cell_row[(long long)y * geo.nx + x];
            if (row >= 0) {
                const R* const ad = sh.ad + (long long)row * 16;
                const unsigned nm = sh.near[row];
#pragma unroll
                for (int k = 1; k < Q; ++k)
                    if ((lw >> (k - 1)) & 1) {   // (shape_link, spelled in place: the call changes the code of every reader kernel)
                        const bool near = (nm >> (k - 1)) & 1u;
                        const R other = src[near ? opp(k) * as.plane + as.at(x + cxk(k), y - cyk(k)) : k * as.plane + as.at(x, y)];
                        g[k] = shape_rule<R>(g[k], other, ad[k - 1], ad[8 + k - 1]);
                    }
            }
        }
    }
    if (sem_is_bb(SEM)) {
        // a source outside [0, nx) x [0, NY): the cell's own post-collision population of the opposite direction; beyond the lid
        // (corner ghosts included) plus the lid term.  The cell's own slots were stored at its own position by update_cell_a (every
        // slot streams); the ghost positions of the pulls above are read but not used here.
        if (x == 0 || x == geo.nx - 1 || gy == 0 || gy == geo.NY - 1) {
#pragma unroll
            for (int k = 1; k < Q; ++k) {
                const int sx = x - cxk(k), sgy = gy + cyk(k);
                if (sx < 0 || sx >= geo.nx || sgy < 0 || sgy >= geo.NY) g[k] = src[opp(k) * as.plane + as.at(x, y)];
            }
            if (gy == 0) {
                const R t = lid_term<R>(src[wall_rho_at(as, geo, x, y, gy)], uLB);
                g[8] = g[8] + t;
                g[7] = g[7] - t;
            }
        }
        return;
    }
    if (x == 0 || x == geo.nx - 1 || gy == 0 || gy == geo.NY - 1) {
        const R rho_w = src[wall_rho_at(as, geo, x, y, gy)];
        R fe[Q];
        equ<R, PROM>(rho_w, gy == 0 ? uLB : (R)0, (R)0, fe);
        wall_rules<R, SEM>(g, fe, x, gy, geo.nx, geo.NY);
    }
}
template <typename R, int SEM, bool PROM = false>
__device__ __forceinline__ void gather(const R* __restrict__ src, const Geo& geo, int raw, R uLB, int x, int y, R (&g)[Q]) {
    gather_a<R, SEM, Geo, PROM>(src, geo, geo, raw, uLB, x, y, g);
}

// One fused update of cell (x, y): gather -> (kept slots) -> moments -> collide -> store.
// as / ad: addressing of the source / destination (Geo = lattice in memory, Window = LDS window of the fused frame passes).
// WALL (SEM_SOLID on a lattice in memory, k_step_generic_wall of lbm_solid.hpp; WALL_REST everywhere else), wa: the mode's tables of the
// cell's lattice.  WALL_MOVE: a cell with links adds the delta of link k to its post-collision population of direction opp(k) before it
// stores it, one add in the lattice type; no gather changes.  WALL_SHAPE: the gather applies shape_rule on the links, the stores are the
// pure post-collision values.  dr: the driving force (k_step_generic_wall alone passes one), added after the collision and before the
// delta of WALL_MOVE, in the raw first step too.
// SGS (k_step_generic_wall in a mode with WALL_SGS alone; WALL is then the base mode), sgs: the sub-grid closure -- w_nu = subgrid_omega of
// the gathered populations and the moments of the cell, k = sgs.
// RLX (k_step_generic_wall in a mode with WALL_RELAX alone), rw, rwm: the cell's own rates of a relaxation field -- rw where the lattice's
// w_nu stands (with SGS: as the closure's omega), rwm as TRT's odd rate.
// RHEO (k_step_generic_wall in a mode with WALL_RHEO alone), rh: the rheology table -- rheology_rates of the gathered populations and the
// moments of the cell give both rates.
template <typename R, int COLL, int SEM, bool TURB, typename AS, typename AD, int WALL = WALL_REST, bool SGS = false, bool RLX = false,
          bool RHEO = false, typename RH = RheoNone>
__device__ __forceinline__ void update_cell_a(const R* __restrict__ src, const AS& as, R* __restrict__ dst, const AD& ad, const Geo& geo,
                                              const Relax<R>& w0, int raw, int x, int y, const R* __restrict__ lnk = nullptr,
                                              WallArg<R, WALL> wa = WallArg<R, WALL>{}, Drive<R> dr = Drive<R>{}, R sgs = R(0), R rw = R(0),
                                              R rwm = R(0), RH rh = RH{}) {
    // lnk (SEM_SOLID with an LDS window as the source): plane K_LINK of the lattice, see link_word
    const int X = geo.nx, Y = geo.NY, gy = geo.y0 + y;
    if (SEM == SEM_SOLID && (link_word<R, AS>(src, as, geo, lnk, x, y) & (LINK_SOLID | LINK_HOLD))) return;   // a solid cell, or a hold cell, is never updated
    R g[Q];
    if constexpr (WALL == WALL_SHAPE) gather_a<R, SEM, AS, coll_is_prom(COLL), true>(src, as, geo, raw, w0.uLB, x, y, g, lnk, wa.sh);
    else gather_a<R, SEM, AS, coll_is_prom(COLL)>(src, as, geo, raw, w0.uLB, x, y, g, lnk);
    // kept slots: a slot outside its streaming window keeps its value; park it where the
    // next pull of this cell will look for it.
    const bool near_edge = (x <= 0) || (x >= X - 2) || (gy <= 0) || (gy >= Y - 2);
    if (near_edge) {
#pragma unroll
        for (int k = 1; k < Q; ++k)
            if (!in_window<SEM>(k, x, gy, X, Y)) dst[k * ad.plane + ad.at(x - cxk(k), y + cyk(k))] = g[k];
    }
    R rho, ux, uy, out[Q], q2 = (R)0;
    const auto me = ad.at(x, y);
    const auto me_s = as.at(x, y);
    const Relax<R>& w = w0;
    R w_nu = w0.w_nu;
    if (TURB) w_nu = smagorinsky_omega<R, coll_is_fast(COLL), coll_is_prom(COLL)>(g, src[K_QEQ * as.plane + me_s], src[K_RHO * as.plane + me_s], w0.w_nu);
    macros<R, coll_is_fast(COLL), SEM>(g, x, gy, X, Y, w.uLB, rho, ux, uy);
    if constexpr (RHEO) {
        R w_m;
        rheology_rates<R, coll_is_fast(COLL)>(g, rho, ux, uy, rh, w0.w_m, w_nu, w_m);
        equ_collide<R, COLL, TURB, true>(g, rho, ux, uy, w, w_nu, out, q2, COLL == C_MRT_FAST && gy == 0 && !sem_is_bb(SEM), w_m);
    } else if constexpr (RLX) {
        w_nu = rw;
        if constexpr (SGS) w_nu = subgrid_omega<R, coll_is_fast(COLL)>(g, rho, ux, uy, rw, sgs);
        equ_collide<R, COLL, TURB, true>(g, rho, ux, uy, w, w_nu, out, q2, COLL == C_MRT_FAST && gy == 0 && !sem_is_bb(SEM), rwm);
    } else {
        if constexpr (SGS) w_nu = subgrid_omega<R, coll_is_fast(COLL)>(g, rho, ux, uy, w0.w_nu, sgs);
        equ_collide<R, COLL, TURB>(g, rho, ux, uy, w, w_nu, out, q2, COLL == C_MRT_FAST && gy == 0 && !sem_is_bb(SEM));
    }
    if (TURB) {
        dst[K_QEQ * ad.plane + me] = q2;
        dst[K_RHO * ad.plane + me] = rho;
    }
    if (dr.on) {
#pragma unroll
        for (int k = 1; k < Q; ++k) out[k] = out[k] + dr.f[k - 1];
    }
    if constexpr (WALL == WALL_MOVE && SEM == SEM_SOLID) {
        const int lw = link_word<R, AS>(src, as, geo, lnk, x, y);
        const int row = (lw & 255) ? wa.cell_row[(long long)y * geo.nx + x] : -1;
        if (row >= 0) {
#pragma unroll
            for (int k = 1; k < Q; ++k)
                if ((lw >> (k - 1)) & 1) out[opp(k)] = out[opp(k)] + wa.delta[(long long)row * 8 + (k - 1)];
        }
    }
    if (!near_edge) {
#pragma unroll
        for (int k = 0; k < Q; ++k) dst[k * ad.plane + me] = out[k];
    } else {
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            // skip the slot if the receiving cell exists but does not stream it (it is that
            // cell's kept slot, written by the receiving cell itself)
            const int dx = x + cxk(k), dgy = gy - cyk(k);
            const bool inside = dx >= 0 && dx < X && dgy >= 0 && dgy < Y;
            if (!inside || in_window<SEM>(k, dx, dgy, X, Y)) dst[k * ad.plane + me] = out[k];
        }
        if (x == 0 || x == X - 1 || gy == 0 || gy == Y - 1) dst[wall_rho_at(ad, geo, x, y, gy)] = rho;
    }
}

template <typename R, int COLL, int SEM, bool TURB = false>
__device__ __forceinline__ void update_cell(const R* __restrict__ src, R* __restrict__ dst, const Geo& geo,
                                            const Relax<R>& w0, int raw, int x, int y) {
    update_cell_a<R, COLL, SEM, TURB, Geo, Geo>(src, geo, dst, geo, geo, w0, raw, x, y);
}

// ------------------------------------------------------------------------------------------
// Vector path (MRT_GPU.py semantics only): a thread owns V consecutive cells of one row and
// moves 16 bytes per direction plane per access.  Rows on the lid / bottom wall are handed
// to update_cell (wall rules, kept slots, parked densities); on every other row the only
// wall cells are x = 0 and x = X-1, where MRT_GPU.py:674-682 reduces exactly to copying
// the opposite population: fe_a - fe_b is +0 for a resting wall (same weight, u = 0), so
// f_a = 0 + f_b.  Arithmetic per cell is the same sequence of IEEE operations as update_cell.
// ------------------------------------------------------------------------------------------
template <typename R, int V>
struct VecT {
    typedef R type __attribute__((ext_vector_type(V)));
};

template <typename R, int V, bool NT>
__device__ __forceinline__ typename VecT<R, V>::type vload(const R* p, bool aligned) {
    typedef typename VecT<R, V>::type T;
    if (aligned) {
        if (NT) return __builtin_nontemporal_load(reinterpret_cast<const T*>(p));
        return *reinterpret_cast<const T*>(p);
    }
    T t;   // element-aligned only (x -+ 1 neighbours): one unaligned 16-byte global load
    __builtin_memcpy(&t, p, sizeof(T));
    return t;
}

template <typename R, int V, bool NT>
__device__ __forceinline__ void vstore(R* p, typename VecT<R, V>::type v) {
    typedef typename VecT<R, V>::type T;
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<T*>(p));
    else *reinterpret_cast<T*>(p) = v;
}

template <typename R, int COLL, int V, bool NT, bool TURB = false>
__device__ __forceinline__ void update_vec(const R* __restrict__ src, R* __restrict__ dst, const Geo& geo,
                                           const Relax<R>& w0, int raw, int x0, int y) {
    typedef typename VecT<R, V>::type T;
    const int X = geo.nx;
    const long long me = geo.at(x0, y);
    T in[Q], outv[Q], hq, hr;
    if (TURB) {
        hq = vload<R, V, NT>(src + K_QEQ * geo.plane + me, true);
        hr = vload<R, V, NT>(src + K_RHO * geo.plane + me, true);
    }
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        const int cx = raw ? 0 : cxk(k), cy = raw ? 0 : cyk(k);
        in[k] = vload<R, V, NT>(src + k * geo.plane + geo.at(x0 - cx, y + cy), cxk(k) == 0 || raw);
    }
#pragma unroll
    for (int c = 0; c < V; ++c) {
        const int x = x0 + c;
        R g[Q], out[Q], q2 = (R)0;
#pragma unroll
        for (int k = 0; k < Q; ++k) g[k] = in[k][c];
        const bool left = (c == 0) && (x == 0), right = (c == V - 1) && (x == X - 1);
        if (!raw) {
            if (left) { g[1] = (R)0 + g[3]; g[5] = (R)0 + g[7]; g[8] = (R)0 + g[6]; }
            if (right) { g[3] = (R)0 + g[1]; g[6] = (R)0 + g[8]; g[7] = (R)0 + g[5]; }
        }
        R w_nu = w0.w_nu;
        if (TURB) w_nu = smagorinsky_omega<R, coll_is_fast(COLL), coll_is_prom(COLL)>(g, hq[c], hr[c], w0.w_nu);
        R rho = ((((((((g[0] + g[1]) + g[2]) + g[3]) + g[4]) + g[5]) + g[6]) + g[7]) + g[8]);
        R ux = (R)0, uy = (R)0;
        if (!coll_is_mrt(COLL) || TURB) {   // the plain MRT operator needs neither u nor feq (MRT_GPU.py:633-648)
            ux = div_<coll_is_fast(COLL)>((((((g[1] - g[3]) + g[5]) - g[6]) - g[7]) + g[8]), rho);
            uy = div_<coll_is_fast(COLL)>((((((g[2] - g[4]) + g[5]) + g[6]) - g[7]) - g[8]), rho);
            if (left || right) { ux = (R)0; uy = (R)0; }
        }
        equ_collide<R, COLL, TURB>(g, rho, ux, uy, w0, w_nu, out, q2);
#pragma unroll
        for (int k = 0; k < Q; ++k) outv[k][c] = out[k];
        if (TURB) { hq[c] = q2; hr[c] = rho; }
    }
#pragma unroll
    for (int k = 0; k < Q; ++k) vstore<R, V, NT>(dst + k * geo.plane + me, outv[k]);
    if (TURB) {
        vstore<R, V, NT>(dst + K_QEQ * geo.plane + me, hq);
        vstore<R, V, NT>(dst + K_RHO * geo.plane + me, hr);
    }
}

// ------------------------------------------------------------------------------------------
// Two time steps per launch on the wall-free interior (temporal blocking through LDS).
//
// A workgroup owns a TX x TY tile of cells that are at least 4 cells away from every wall and
// slab edge.  Phase 1 performs step n -> n+1 for the tile plus a one-cell rim (rounded out to
// whole vectors in x: TX + 2V columns, TY + 2 rows), pulling from global memory, and leaves the
// post-collision populations in LDS; phase 2 performs step n+1 -> n+2 for the tile, pulling from
// LDS, and stores to global memory.  HBM traffic per cell and step drops from 18 words to about
// (9 * 1.39 + 9) / 2 = 10.8.  No wall logic is needed: every cell whose value is used is an
// ordinary cell in both semantics (MRT.py windows and kept slots only involve cells within two
// cells of a wall).  Rim cells that phase 2 does not use may be computed from ghost/pad data and
// hold garbage -- harmless.  Per-cell arithmetic is the same operation sequence as update_cell,
// so the result is bit-identical to two single steps.
// ------------------------------------------------------------------------------------------
template <typename R, int COLL, int V, bool TURB, bool SGS = false, bool RLX = false, bool RHEO = false, typename RH = RheoNone>
__device__ __forceinline__ void collide_vec(const typename VecT<R, V>::type (&in)[Q], const Relax<R>& w0,
                                            typename VecT<R, V>::type (&outv)[Q],
                                            typename VecT<R, V>::type& hq, typename VecT<R, V>::type& hr, bool wl = false, bool wr = false,
                                            int kind = 0, R sgs = R(0), typename VecT<R, V>::type rw = typename VecT<R, V>::type{},
                                            typename VecT<R, V>::type rwm = typename VecT<R, V>::type{}, RH rh = RH{}) {
    // RHEO (k_step_solid in a mode with WALL_RHEO alone, kind 0): rh, the rheology table -- rheology_rates of the cell's populations and
    // moments give both rates (the packed halves gather per half); the MRT operators then form the velocity too
    // RLX (k_step_solid in a mode with WALL_RELAX alone, kind 0): rw, rwm -- the V cells' own rates of a relaxation field, in the lane
    // order of in[k] (the packed halves p = 0 / 1 take .xy / .zw of them as they do of in[k]): rw where the lattice's w_nu stands (with
    // SGS: as the closure's omega), rwm as TRT's odd rate
    // SGS (k_step_solid in a mode with WALL_SGS alone, kind 0): the sub-grid closure, w_nu = subgrid_omega of the cell's populations and
    // moments with k = sgs -- the MRT operators then form the velocity too
    // hq, hr: Smagorinsky history of the cells (in: previous step, out: this step); untouched unless TURB
    // The streaming kernel with the walls inside (lbm_stream.hpp) passes wall cells, their wall rules already applied to in[]:
    // wl / wr: the first / last cell is a side-wall cell (x = 0 / X - 1): u = 0 (MRT_GPU.py:396-399; as update_vec);
    // kind 1: the V cells are lid cells -- rho = (f0+f1+f3) + 2 (f2+f5+f6), u = (uLB, 0) (MRT_GPU.py:400-405); kind 2: bottom-wall
    // cells, u = 0
    if constexpr (sizeof(R) == 4 && V == 4) {
        // fp32: two cells per operation (packed math), same lane-wise IEEE operations as the scalar form below
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            f32x2 g[Q], out[Q], q2 = f32x2(0.f);
#pragma unroll
            for (int k = 0; k < Q; ++k) g[k] = p == 0 ? in[k].xy : in[k].zw;
            f32x2 w_nu = (f32x2)(w0.w_nu);
            if (TURB) w_nu = smagorinsky_omega<f32x2, coll_is_fast(COLL), coll_is_prom(COLL)>(g, p == 0 ? hq.xy : hq.zw, p == 0 ? hr.xy : hr.zw, w0.w_nu);
            f32x2 rho = ((((((((g[0] + g[1]) + g[2]) + g[3]) + g[4]) + g[5]) + g[6]) + g[7]) + g[8]);
            if (kind == 1) rho = ((g[0] + g[1]) + g[3]) + 2.f * ((g[2] + g[5]) + g[6]);
            f32x2 ux = f32x2(0.f), uy = f32x2(0.f);
            if (!coll_is_mrt(COLL) || TURB || SGS || RHEO) {
                if (kind == 0) {
                    ux = div_<coll_is_fast(COLL)>((((((g[1] - g[3]) + g[5]) - g[6]) - g[7]) + g[8]), rho);
                    uy = div_<coll_is_fast(COLL)>((((((g[2] - g[4]) + g[5]) + g[6]) - g[7]) - g[8]), rho);
                    if (wl && p == 0) { ux.x = 0.f; uy.x = 0.f; }
                    if (wr && p == 1) { ux.y = 0.f; uy.y = 0.f; }
                } else {
                    ux = f32x2(kind == 1 ? w0.uLB : 0.f); uy = f32x2(0.f);
                }
            }
            if constexpr (RHEO) {
                f32x2 w_m;
                rheology_rates<f32x2, coll_is_fast(COLL)>(g, rho, ux, uy, rh, w0.w_m, w_nu, w_m);
                equ_collide<f32x2, COLL, TURB, true>(g, rho, ux, uy, w0, w_nu, out, q2, COLL == C_MRT_FAST && kind == 1, w_m);
            } else if constexpr (RLX) {
                const f32x2 rwp = p == 0 ? rw.xy : rw.zw, rmp = p == 0 ? rwm.xy : rwm.zw;
                w_nu = rwp;
                if constexpr (SGS) w_nu = subgrid_omega<f32x2, coll_is_fast(COLL), f32x2>(g, rho, ux, uy, rwp, sgs);
                equ_collide<f32x2, COLL, TURB, true>(g, rho, ux, uy, w0, w_nu, out, q2, COLL == C_MRT_FAST && kind == 1, rmp);
            } else {
                if constexpr (SGS) w_nu = subgrid_omega<f32x2, coll_is_fast(COLL)>(g, rho, ux, uy, w0.w_nu, sgs);
                equ_collide<f32x2, COLL, TURB>(g, rho, ux, uy, w0, w_nu, out, q2, COLL == C_MRT_FAST && kind == 1);
            }
#pragma unroll
            for (int k = 0; k < Q; ++k) {
                if (p == 0) outv[k].xy = out[k];
                else outv[k].zw = out[k];
            }
            if (TURB) {
                if (p == 0) { hq.xy = q2; hr.xy = rho; }
                else { hq.zw = q2; hr.zw = rho; }
            }
#ifdef LBM_SEQ_HALVES
            if (p == 0) __builtin_amdgcn_sched_barrier(0);   // (experiment: the two halves one after the other -- fewer live temporaries)
#endif
        }
    } else {
#pragma unroll
        for (int c = 0; c < V; ++c) {
            R g[Q], out[Q], q2 = (R)0;
#pragma unroll
            for (int k = 0; k < Q; ++k) g[k] = in[k][c];
            R w_nu = w0.w_nu;
            if (TURB) w_nu = smagorinsky_omega<R, coll_is_fast(COLL), coll_is_prom(COLL)>(g, hq[c], hr[c], w0.w_nu);
            R rho = ((((((((g[0] + g[1]) + g[2]) + g[3]) + g[4]) + g[5]) + g[6]) + g[7]) + g[8]);
            if (kind == 1) rho = ((g[0] + g[1]) + g[3]) + (R)2. * ((g[2] + g[5]) + g[6]);
            R ux = (R)0, uy = (R)0;
            if (!coll_is_mrt(COLL) || TURB || SGS || RHEO) {
                if (kind == 0) {
                    ux = div_<coll_is_fast(COLL)>((((((g[1] - g[3]) + g[5]) - g[6]) - g[7]) + g[8]), rho);
                    uy = div_<coll_is_fast(COLL)>((((((g[2] - g[4]) + g[5]) + g[6]) - g[7]) - g[8]), rho);
                    if ((wl && c == 0) || (wr && c == V - 1)) { ux = (R)0; uy = (R)0; }
                } else {
                    ux = kind == 1 ? w0.uLB : (R)0; uy = (R)0;
                }
            }
            if constexpr (RHEO) {
                R w_m;
                rheology_rates<R, coll_is_fast(COLL)>(g, rho, ux, uy, rh, w0.w_m, w_nu, w_m);
                equ_collide<R, COLL, TURB, true>(g, rho, ux, uy, w0, w_nu, out, q2, COLL == C_MRT_FAST && kind == 1, w_m);
            } else if constexpr (RLX) {
                w_nu = rw[c];
                if constexpr (SGS) w_nu = subgrid_omega<R, coll_is_fast(COLL)>(g, rho, ux, uy, rw[c], sgs);
                equ_collide<R, COLL, TURB, true>(g, rho, ux, uy, w0, w_nu, out, q2, COLL == C_MRT_FAST && kind == 1, rwm[c]);
            } else {
                if constexpr (SGS) w_nu = subgrid_omega<R, coll_is_fast(COLL)>(g, rho, ux, uy, w0.w_nu, sgs);
                equ_collide<R, COLL, TURB>(g, rho, ux, uy, w0, w_nu, out, q2, COLL == C_MRT_FAST && kind == 1);
            }
#pragma unroll
            for (int k = 0; k < Q; ++k) outv[k][c] = out[k];
            if (TURB) { hq[c] = q2; hr[c] = rho; }
        }
    }
}

template <typename R, int COLL, int V, int TX, int TY, int NT, bool TURB>
__device__ __forceinline__ void update_tile2(const R* __restrict__ src, R* __restrict__ dst, const Geo& geo,
                                             const Relax<R>& w, R* __restrict__ lds, int tx0, int ty0, int xe, int ye) {
    typedef typename VecT<R, V>::type T;
    constexpr int PW = TX + 2 * V, PH = TY + 2, PVC = PW / V, TVC = TX / V;
    // phase 1: rows ty0-1 .. ty0+TY, columns tx0-V .. tx0+TX+V-1  ->  lds[Q (+2)][PH][PW]
    for (int i = threadIdx.x; i < PH * PVC; i += NT) {
        const int r = i / PVC, vc = i - r * PVC;
        const int x0 = tx0 - V + vc * V, y = ty0 - 1 + r;
        if (x0 < geo.nx && y < geo.ny) {
            T in[Q], outv[Q], hq, hr;
#pragma unroll
            for (int k = 0; k < Q; ++k)
                in[k] = vload<R, V, false>(src + k * geo.plane + geo.at(x0 - cxk(k), y + cyk(k)), cxk(k) == 0);
            if (TURB) {
                hq = vload<R, V, false>(src + K_QEQ * geo.plane + geo.at(x0, y), true);
                hr = vload<R, V, false>(src + K_RHO * geo.plane + geo.at(x0, y), true);
            }
            collide_vec<R, COLL, V, TURB>(in, w, outv, hq, hr);
#pragma unroll
            for (int k = 0; k < Q; ++k) *reinterpret_cast<T*>(lds + ((k * PH + r) * PW + vc * V)) = outv[k];
            if (TURB) {
                *reinterpret_cast<T*>(lds + ((K_QEQ * PH + r) * PW + vc * V)) = hq;
                *reinterpret_cast<T*>(lds + ((K_RHO * PH + r) * PW + vc * V)) = hr;
            }
        }
    }
    __syncthreads();
    // phase 2: the tile itself, pulling from LDS
    for (int i = threadIdx.x; i < TY * TVC; i += NT) {
        const int r = i / TVC, vc = i - r * TVC;
        const int x0 = tx0 + vc * V, y = ty0 + r;
        if (x0 >= xe || y >= ye) continue;
        T in[Q], outv[Q], hq, hr;
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            // one aligned 16-byte LDS read of the thread's own columns + ONE scalar for the x -+ 1 neighbour
            // (V scalar reads at a stride of V words are a V-way bank conflict)
            const R* p = lds + ((k * PH + (r + 1 + cyk(k))) * PW + (V + vc * V));
            const T own = *reinterpret_cast<const T*>(p);
            if (cxk(k) == 0) {
                in[k] = own;
            } else if (cxk(k) > 0) {
                in[k][0] = p[-1];
#pragma unroll
                for (int c = 1; c < V; ++c) in[k][c] = own[c - 1];
            } else {
#pragma unroll
                for (int c = 0; c < V - 1; ++c) in[k][c] = own[c + 1];
                in[k][V - 1] = p[V];
            }
        }
        if (TURB) {
            hq = *reinterpret_cast<const T*>(lds + ((K_QEQ * PH + (r + 1)) * PW + (V + vc * V)));
            hr = *reinterpret_cast<const T*>(lds + ((K_RHO * PH + (r + 1)) * PW + (V + vc * V)));
        }
        collide_vec<R, COLL, V, TURB>(in, w, outv, hq, hr);
        const long long me = geo.at(x0, y);
#pragma unroll
        for (int k = 0; k < Q; ++k) vstore<R, V, false>(dst + k * geo.plane + me, outv[k]);
        if (TURB) {
            vstore<R, V, false>(dst + K_QEQ * geo.plane + me, hq);
            vstore<R, V, false>(dst + K_RHO * geo.plane + me, hr);
        }
    }
}

// ------------------------------------------------------------------------------------------
// S time steps per launch with ONE LDS buffer updated in place (used with S = 3, the default
// without the Smagorinsky closure: profiles/r01_logs/perf11.log).  One vector cell per thread: the region is PH = TY + 2(S-1) rows
// by PW = TX + 2V columns and the workgroup has PH * PW / V threads.  Step 1 pulls from global
// memory; steps 2..S pull from LDS into registers, wait for everyone, compute, and overwrite
// their own slot; the region that is still valid shrinks by one cell per step (the V-wide rim in
// x allows up to V + 1 steps).  Threads outside the valid region compute garbage that nobody uses.
// ------------------------------------------------------------------------------------------
// LDS holds only the six directions that cross rows (k = 2, 4, 5, 6, 7, 8); the three that stay in the row are taken
// from the thread's own registers (k = 0) and from the neighbouring lanes' registers by a wave shuffle (k = 1, 3: the row of
// PVC vector cells sits in PVC consecutive lanes).  Two thirds of the LDS footprint -> three workgroups per CU.
constexpr int TB_LDS_PLANES = 6;
__host__ __device__ constexpr int lds_slot(int k) { return k == 2 ? 0 : k == 4 ? 1 : k - 3; }   // 5,6,7,8 -> 2,3,4,5

// SOLID (SEM_SOLID, off in every other instantiation): the lattice has solid cells.  The rule is cell-local -- a slot whose source is a
// solid cell takes the cell's OWN post-collision population of the opposite direction -- and the thread keeps its cells' post-collision
// populations outv[] in registers for all S steps, so a solid link costs no LDS or memory traffic from step 2 on: a select between
// in[k] and outv[opp(k)].  The thread reads the V link words of its cells once (rim cells included: they can be solid or next to a solid
// cell and are recomputed like every cell of the shrinking region) and keeps them packed in two registers for the launch: the eight link
// bits of each cell in `links`, the "solid" bit of each cell in `solid`.  Step 1: the pull from `src`, then one more aligned load of the
// thread's own vector per direction that has a link in one of its cells.  Solid lanes compute garbage and are overwritten with w_k
// after every collision: they hold the rest equilibrium in LDS, in the shuffles and in the stores, the constants k_solid_fix wrote.
// The arithmetic stays collide_vec: the same bits as k_step_generic<.., SEM_SOLID> applied S times.
template <typename R, int V>
__device__ __forceinline__ void solid_lanes(typename VecT<R, V>::type (&outv)[Q], unsigned solid) {
#pragma unroll
    for (int c = 0; c < V; ++c)
        if ((solid >> c) & 1u) {
#pragma unroll
            for (int k = 0; k < Q; ++k) outv[k][c] = weight<R>(k);
        }
}

template <typename R, int COLL, int V, int TX, int TY, int S, bool TURB, int RV = 1, bool SOLID = false>
__device__ __forceinline__ void update_tile_inplace(const R* __restrict__ src, R* __restrict__ dst, const Geo& geo,
                                                    const Relax<R>& w, R* __restrict__ lds, int tx0, int ty0, int xe, int ye) {
    // RV: vector cells of rim on each side in x (fp64 vectors hold two cells: more than three steps need two of them)
    typedef typename VecT<R, V>::type T;
    static_assert(!(SOLID && TURB), "no closure with solid cells");
    unsigned links = 0, solid = 0;   // SOLID: bits 8 c .. 8 c + 7 = the link bits of cell c; bit c = cell c is solid
    constexpr int PW = TX + 2 * RV * V, PH = TY + 2 * (S - 1), PVC = PW / V;
    static_assert(S - 1 <= RV * V, "the x rim is RV * V cells wide");
    static_assert(64 % PVC == 0, "a row of vector cells must not straddle two waves");
    const int r = threadIdx.x / PVC, vc = threadIdx.x % PVC;
    const int x0 = tx0 - RV * V + vc * V, y = ty0 - (S - 1) + r;
    T in[Q], outv[Q], hq, hr;
    const bool inside = x0 < geo.nx && y < geo.ny;
    if (inside) {
#pragma unroll
        for (int k = 0; k < Q; ++k)
            in[k] = vload<R, V, false>(src + k * geo.plane + geo.at(x0 - cxk(k), y + cyk(k)), cxk(k) == 0);
        if (TURB) {   // the Smagorinsky history is cell-local: it stays in this thread's registers for all S steps
            hq = vload<R, V, false>(src + K_QEQ * geo.plane + geo.at(x0, y), true);
            hr = vload<R, V, false>(src + K_RHO * geo.plane + geo.at(x0, y), true);
        }
        if constexpr (SOLID) {
            const long long me = geo.at(x0, y);
            const T lk = vload<R, V, false>(src + K_LINK * geo.plane + me, true);
#pragma unroll
            for (int c = 0; c < V; ++c) {
                const unsigned lw = (unsigned)(int)lk[c];
                links |= (lw & 255u) << (8 * c);
                solid |= ((lw >> 8) & 1u) << c;
            }
            if (links) {
#pragma unroll
                for (int k = 1; k < Q; ++k) {
                    if (!(links & (0x01010101u << (k - 1)))) continue;
                    const T own = vload<R, V, false>(src + opp(k) * geo.plane + me, true);
#pragma unroll
                    for (int c = 0; c < V; ++c)
                        if ((links >> (8 * c + k - 1)) & 1u) in[k][c] = own[c];
                }
            }
        }
        collide_vec<R, COLL, V, TURB>(in, w, outv, hq, hr);
        if constexpr (SOLID) {
            if (solid) solid_lanes<R, V>(outv, solid);
        }
    }
#pragma unroll
    for (int s = 2; s <= S; ++s) {
        if (inside) {
#pragma unroll
            for (int k = 0; k < Q; ++k)
                if (cyk(k) != 0) *reinterpret_cast<T*>(lds + ((lds_slot(k) * PH + r) * PW + vc * V)) = outv[k];
        }
        // the in-row directions never leave the registers: east-moving values come from the left neighbour's last
        // element, west-moving ones from the right neighbour's first (garbage at the two rim columns, which is fine)
        const R from_left = __shfl_up(outv[1][V - 1], 1);
        const R from_right = __shfl_down(outv[3][0], 1);
        __syncthreads();
        const bool act = r >= s - 1 && r < PH - (s - 1);
        if (act) {
            in[0] = outv[0];
            in[1][0] = from_left;
            in[3][V - 1] = from_right;
#pragma unroll
            for (int c = 1; c < V; ++c) { in[1][c] = outv[1][c - 1]; in[3][c - 1] = outv[3][c]; }
#pragma unroll
            for (int k = 0; k < Q; ++k) {
                if (cyk(k) == 0) continue;
                const R* p = lds + ((lds_slot(k) * PH + (r + cyk(k))) * PW + vc * V);
                const T own = *reinterpret_cast<const T*>(p);
                if (cxk(k) == 0) {
                    in[k] = own;
                } else if (cxk(k) > 0) {
                    in[k][0] = p[-1];
#pragma unroll
                    for (int c = 1; c < V; ++c) in[k][c] = own[c - 1];
                } else {
#pragma unroll
                    for (int c = 0; c < V - 1; ++c) in[k][c] = own[c + 1];
                    in[k][V - 1] = p[V];
                }
            }
        }
        if (s < S) __syncthreads();   // everyone has read before anyone overwrites in place
        // (the rim columns are needed by the next step but not after the last one)
        if (act && (s < S || (vc >= RV && vc < PVC - RV))) {
            if constexpr (SOLID) {
                // outv still holds this thread's post-collision populations of the step before.  Threads without a link skip the selects
                // (most of a lattice with few obstacles), except in the strict fp64 TRT variant: with the branch its S = 4 and S = 5 kernels
                // need 16 B of scratch under the 128 registers of the occupancy floor, without it 121 registers and none
                constexpr bool SKIP = !(sizeof(R) == 8 && COLL == C_TRT);
                if (!SKIP || links) {
#pragma unroll
                    for (int k = 1; k < Q; ++k) {
#pragma unroll
                        for (int c = 0; c < V; ++c)
                            if ((links >> (8 * c + k - 1)) & 1u) in[k][c] = outv[opp(k)][c];
                    }
                }
            }
            collide_vec<R, COLL, V, TURB>(in, w, outv, hq, hr);
            if constexpr (SOLID) {
                if (solid) solid_lanes<R, V>(outv, solid);
            }
        }
    }
    if (r >= S - 1 && r < PH - (S - 1) && vc >= RV && vc < PVC - RV && x0 < xe && y < ye) {
        const long long me = geo.at(x0, y);
#pragma unroll
        for (int k = 0; k < Q; ++k) vstore<R, V, false>(dst + k * geo.plane + me, outv[k]);
        if (TURB) {
            vstore<R, V, false>(dst + K_QEQ * geo.plane + me, hq);
            vstore<R, V, false>(dst + K_RHO * geo.plane + me, hr);
        }
    }
}

}  // namespace lbm
