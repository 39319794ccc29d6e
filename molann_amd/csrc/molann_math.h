// molann_math.h - per-frame arithmetic of the molann forward path, written once as
// __host__ __device__ code: the gfx950 kernels inline it, and the molann_selftest_* hooks compile the
// same source for the host so the CPU test-suite can check it against the oracle.
//
//   features      molann/ann.py:323-354   (angle / bond / dihedral / position)
//   kabsch        molann/ann.py:187-195   (rotation from the 3x3 covariance)
//   activations   molann/ann.py:37,64     (the module placed between the Linear layers)
#pragma once

#if !defined(__HIPCC_RTC__) // hipRTC provides the runtime declarations and libm itself
#include <hip/hip_runtime.h>
#include <math.h>
#endif

#define MOLANN_HD __host__ __device__ __forceinline__

namespace molann {

// item types of the expanded feature table (one output column group each)
enum ItemType : int {
    IT_ANGLE_COS = 0,   // ann.py:328-332, use_angle_value = False
    IT_BOND = 1,        // ann.py:334-336
    IT_DIHEDRAL_CS = 2, // ann.py:344-351, [cos, sin]
    IT_POSITION = 3,    // ann.py:353-354, one atom (3 columns); a k-atom feature is k items
    IT_ANGLE_VAL = 4,   // ann.py:330 acos
    IT_DIHEDRAL_VAL = 5 // ann.py:349 atan2
};

struct V3 {
    float x, y, z;
};

MOLANN_HD V3 v3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
MOLANN_HD V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
MOLANN_HD V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
MOLANN_HD float dot(V3 a, V3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
MOLANN_HD V3 cross(V3 a, V3 b) {
    return v3(fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x)));
}

// ---- fast scalar helpers (device: one hardware instruction; host: libm) -----------------------
MOLANN_HD float fast_rcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);
#else
    return 1.0f / x;
#endif
}
MOLANN_HD float fast_rsq(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rsqf(x);
#else
    return 1.0f / sqrtf(x);
#endif
}
// sqrt(x) as x * rsq(x) (1-2 ulp): exact 0 at 0 like sqrtf, NaN for negative / NaN input
MOLANN_HD float fast_sqrt(float x) { return x == 0.0f ? 0.0f : x * fast_rsq(x); }
MOLANN_HD float fast_exp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __expf(x);
#else
    return expf(x);
#endif
}

// ---- features ---------------------------------------------------------------------------------
// bond length |x2 - x1| (ann.py:335-336)
MOLANN_HD float feat_bond(V3 a0, V3 a1) {
    V3 r = a1 - a0;
    return fast_sqrt(dot(r, r));
}

// cosine of the angle at the SECOND atom (ann.py:324-328); no clamp, as in the reference
MOLANN_HD float feat_angle_cos(V3 a0, V3 a1, V3 a2) {
    V3 r21 = a0 - a1;
    V3 r23 = a2 - a1;
    // dot / (|r21| |r23|) with one reciprocal square root of the product of the squared lengths
    return dot(r21, r23) * fast_rsq(dot(r21, r21) * dot(r23, r23));
}

// unnormalised (cos, sin) of the dihedral 1-2-3-4 (ann.py:339-345)
MOLANN_HD void feat_dihedral_raw(V3 a0, V3 a1, V3 a2, V3 a3, float& c, float& s) {
    V3 r12 = a1 - a0;
    V3 r23 = a2 - a1;
    V3 r34 = a3 - a2;
    V3 n1 = cross(r12, r23);
    V3 n2 = cross(r23, r34);
    c = dot(n1, n2);
    s = dot(n1, r34) * fast_sqrt(dot(r23, r23));
}

// One item of the feature table on up to four atoms; writes 1..3 values, returns how many.
MOLANN_HD int eval_item(int type, V3 a0, V3 a1, V3 a2, V3 a3, float (&out)[3]) {
    switch (type) {
    case IT_ANGLE_COS:
        out[0] = feat_angle_cos(a0, a1, a2);
        return 1;
    case IT_ANGLE_VAL: {
        // ann.py:330 takes acos of the cosine, which turns the cosine's rounding into eps / sin(theta) and is NaN once it rounds past
        // +-1.  atan2(|u x v|, u.v) is the same angle with the rounding of its arguments only, at every angle.
        const V3 u = a0 - a1, v = a2 - a1, w = cross(u, v);
        out[0] = atan2f(fast_sqrt(dot(w, w)), dot(u, v));
        return 1;
    }
    case IT_BOND:
        out[0] = feat_bond(a0, a1);
        return 1;
    case IT_DIHEDRAL_CS: {
        float c, s;
        feat_dihedral_raw(a0, a1, a2, a3, c, s);
        const float inv_radius = fast_rsq(fmaf(c, c, s * s)); // 1 / radius, ann.py:346
        out[0] = c * inv_radius;                              // ann.py:351 cos first, then sin
        out[1] = s * inv_radius;
        return 2;
    }
    case IT_DIHEDRAL_VAL: {
        float c, s;
        feat_dihedral_raw(a0, a1, a2, a3, c, s);
        out[0] = atan2f(s, c); // ann.py:349
        return 1;
    }
    default: // IT_POSITION
        out[0] = a0.x;
        out[1] = a0.y;
        out[2] = a0.z;
        return 3;
    }
}

MOLANN_HD int item_width(int type) { return type == IT_POSITION ? 3 : (type == IT_DIHEDRAL_CS ? 2 : 1); }
MOLANN_HD int item_atoms(int type) {
    return (type == IT_BOND) ? 2 : (type == IT_POSITION) ? 1 : (type == IT_ANGLE_COS || type == IT_ANGLE_VAL) ? 3 : 4;
}

// ---- activations ------------------------------------------------------------------------------
// tanh(x) = 1 - 2 / (1 + e^{2x}): five instructions, two of them transcendental.  Absolute error
// <= ~1.5e-7 everywhere (the 1 - 2r cancellation near 0 costs relative, not absolute, accuracy; the
// parity bar of this path is absolute, 1e-5).  +-inf and NaN behave like tanhf.
MOLANN_HD float act_tanh(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float t = __builtin_amdgcn_exp2f(x * 2.88539008177792681472f); // e^{2x} = 2^{2x log2 e}
#else
    const float t = exp2f(x * 2.88539008177792681472f);
#endif
    return fmaf(-2.0f, fast_rcp(1.0f + t), 1.0f);
}

MOLANN_HD float act_sigmoid(float x) { return fast_rcp(1.0f + fast_exp(-x)); }

MOLANN_HD float apply_activation(int act, float v) {
    switch (act) {
    case 0: return act_tanh(v);                       // torch.nn.Tanh (the default, ann.py:37)
    case 1: return fmaxf(v, 0.0f) + (v != v ? v : 0.0f); // ReLU, NaN-propagating like torch
    case 2: return act_sigmoid(v);                    // Sigmoid
    case 3: return v;                                 // Identity
    case 4: return v > 0.0f ? v : expm1f(v);          // ELU(alpha=1)
    case 5: return v * act_sigmoid(v);                // SiLU
    case 6: return v > 20.0f ? v : log1pf(expf(v));   // Softplus(beta=1, threshold=20)
    case 7: return v > 0.0f ? v : 0.01f * v;          // LeakyReLU(0.01)
    case 8: return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); // GELU (erf)
    default: return v;
    }
}

// ---- Kabsch rotation --------------------------------------------------------------------------
// Input: H[a][b] = sum_i p_i[a] * ref_i[b] over the align atoms (p centred frame coordinates, ref the
// reference as the plan packs it, centred whatever the buffer holds) = `prod` of ann.py:187, accumulated in fp64 by the callers (the products of fp32
// coordinates are exact in fp64, so H carries no rounding of its own), and
// e0 >= (sum|p|^2 + sum|ref|^2)/2, an upper bound on the largest eigenvalue used as the Newton start.
// Output: R (row-major) with aligned_row = p_row . R, equal to U diag(1,1,sign det(U Vh)) Vh of
// ann.py:188-195.
//
// Method (not the reference's LAPACK SVD): the optimal proper rotation is the top eigenvector of
// Horn's symmetric 4x4 matrix K(H) read as a unit quaternion.  Its eigenvalues are
// {s1+s2+d*s3, s1-s2-d*s3, -s1+s2-d*s3, -s1-s2+d*s3} (s = singular values, d = sign det H), so the top
// one is simple exactly when the rotation is well defined (s2 + d*s3 > 0): rank-2 covariances (planar
// reference, three align atoms) and reflections need no special case.  lambda_max by Newton on the
// characteristic quartic from above (monotone), eigenvector = the column of adj(K - lambda I) with the
// largest diagonal entry.  fp64 throughout: ~250 flops per frame, against ~60 flops to form H.
MOLANN_HD float tfma(float a, float b, float c) { return fmaf(a, b, c); }
MOLANN_HD double tfma(double a, double b, double c) { return fma(a, b, c); }
MOLANN_HD float tabs(float a) { return fabsf(a); }
MOLANN_HD double tabs(double a) { return fabs(a); }

// T = double: what every plan with position items (and AlignmentLayer.forward) uses.  T = float: the same
// algorithm at the reference's own precision (its SVD runs in fp32) for plans whose items are all invariant
// under rigid motion (bond / angle / dihedral): their outputs do not depend on how accurate R is, only on R
// being a proper rotation, which the normalised quaternion guarantees in either precision.
template <typename T, typename RT = float>
MOLANN_HD void kabsch_rotation_t(const T (&H)[9], T e0, RT (&R)[9]) {
    constexpr bool F32 = sizeof(T) == 4;
    const T tiny = F32 ? (T)1e-30f : (T)1e-30, huge = F32 ? (T)1e30f : (T)1e30;
    T fro2 = (T)0;
#pragma unroll
    for (int i = 0; i < 9; ++i) fro2 = tfma(H[i], H[i], fro2);
    if (!(fro2 > tiny) || !(fro2 < huge)) { // zero / non-finite covariance: no rotation
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? (RT)1 : (RT)0;
        return;
    }
    // scale so that |h|_F ~= 1: the rotation does not depend on the scale, so an fp32 rsqrt is enough
#if defined(__HIP_DEVICE_COMPILE__)
    const T s = (T)__builtin_amdgcn_rsqf((float)fro2);
#else
    const T s = (T)(1.0f / sqrtf((float)fro2));
#endif
    const T hxx = H[0] * s, hxy = H[1] * s, hxz = H[2] * s;
    const T hyx = H[3] * s, hyy = H[4] * s, hyz = H[5] * s;
    const T hzx = H[6] * s, hzy = H[7] * s, hzz = H[8] * s;

    const T k00 = hxx + hyy + hzz, k01 = hyz - hzy, k02 = hzx - hxz, k03 = hxy - hyx;
    const T k11 = hxx - hyy - hzz, k12 = hxy + hyx, k13 = hzx + hxz;
    const T k22 = -hxx + hyy - hzz, k23 = hyz + hzy;
    const T k33 = -hxx - hyy + hzz;

    // characteristic polynomial l^4 + c2 l^2 + c1 l + c0 (trace K = 0)
    const T c2 = (T)-2 * (hxx * hxx + hxy * hxy + hxz * hxz + hyx * hyx + hyy * hyy + hyz * hyz + hzx * hzx +
                              hzy * hzy + hzz * hzz);
    const T det_h = hxx * (hyy * hzz - hyz * hzy) - hxy * (hyx * hzz - hyz * hzx) + hxz * (hyx * hzy - hyy * hzx);
    const T c1 = (T)-8 * det_h;
    T c0;
    {
        const T s0 = k00 * k11 - k01 * k01, s1 = k00 * k12 - k01 * k02, s2 = k00 * k13 - k01 * k03;
        const T s3 = k01 * k12 - k11 * k02, s4 = k01 * k13 - k11 * k03, s5 = k02 * k13 - k12 * k03;
        const T d5 = k22 * k33 - k23 * k23, d4 = k12 * k33 - k13 * k23, d3 = k12 * k23 - k13 * k22;
        const T d2 = k02 * k33 - k03 * k23, d1 = k02 * k23 - k03 * k22, d0 = k02 * k13 - k03 * k12;
        c0 = s0 * d5 - s1 * d4 + s2 * d3 + s3 * d2 - s4 * d1 + s5 * d0;
    }

    // Newton from above; lambda_max <= s1+s2+s3 <= sqrt(3) |h|_F and <= e0 * s
    constexpr T sqrt3 = (T)1.7320508075688772;
    T lam0 = e0 * s < sqrt3 ? e0 * s : sqrt3;
    if (!(lam0 > (T)0)) lam0 = sqrt3;
    // A frame that resembles the reference starts within ~1e-2 of the root (e0 is then tight) and Newton converges
    // quadratically: NFIX unconditional steps - straight-line code, no exec-mask bookkeeping, nothing for the compiler
    // to split into blocks - leave the last step below the tolerance.  Whatever has not converged by then (or went
    // non-finite) takes the guarded loop below; a wave skips it when all its frames are done.
    constexpr int NFIX = F32 ? 4 : 5;
    const T tol = F32 ? (T)1e-6f : (T)1e-14;
    T lam = lam0, step = (T)0;
#pragma unroll
    for (int it = 0; it < NFIX; ++it) {
        const T l2 = lam * lam;
        const T p = tfma(l2 + c2, l2, tfma(c1, lam, c0));
        const T dp = tfma(tfma((T)4, l2, (T)2 * c2), lam, c1);
        step = p * (T)fast_rcp((float)dp);   // Newton corrects itself: an fp32-accurate reciprocal is enough
        lam = lam - step;
    }
    bool done = (step == step) && (tabs(lam) < (T)4) && !(tabs(step) > tol * tabs(lam));
#if defined(__HIP_DEVICE_COMPILE__)
    if (!__all(done)) {
#else
    if (!done) {
#endif
        if (!done && !((lam == lam) && lam > (T)0 && lam <= lam0)) lam = lam0;   // left the monotone path: start again
        // bounded: every lane reaches the exit.  fp32: the residual's own rounding (~1e-7 / p'(lam)) keeps an
        // ill-conditioned frame from ever meeting the step test, so the cap is what ends it there.
#pragma unroll 1
        for (int it = 0; it < (F32 ? 12 : 48); ++it) {
            if (!done) {
                const T l2 = lam * lam;
                const T p = (l2 + c2) * l2 + c1 * lam + c0;
                const T dp = ((T)4 * l2 + (T)2 * c2) * lam + c1;
                const T st = p * (T)fast_rcp((float)dp);
                const T nl = lam - st;
                const bool finite = (st == st) && (tabs(nl) < (T)4);
                if (finite) lam = nl;
                if (!finite || !(tabs(st) > tol * tabs(nl))) done = true;
            }
#if defined(__HIP_DEVICE_COMPILE__)
            if (__all(done)) break; // wave-uniform exit
#else
            if (done) break;
#endif
        }
    }

    // adj(K - lam I) = const * q q^T
    const T m00 = k00 - lam, m11 = k11 - lam, m22 = k22 - lam, m33 = k33 - lam;
    const T s0 = m00 * m11 - k01 * k01, s1 = m00 * k12 - k01 * k02, s2 = m00 * k13 - k01 * k03;
    const T s3 = k01 * k12 - m11 * k02, s4 = k01 * k13 - m11 * k03, s5 = k02 * k13 - k12 * k03;
    const T d5 = m22 * m33 - k23 * k23, d4 = k12 * m33 - k13 * k23, d3 = k12 * k23 - k13 * m22;
    const T d2 = k02 * m33 - k03 * k23, d1 = k02 * k23 - k03 * m22;
    const T a00 = m11 * d5 - k12 * d4 + k13 * d3;
    const T a01 = -k01 * d5 + k02 * d4 - k03 * d3;
    const T a02 = k13 * s5 - k23 * s4 + m33 * s3;
    const T a03 = -k12 * s5 + m22 * s4 - k23 * s3;
    const T a11 = m00 * d5 - k02 * d2 + k03 * d1;
    const T a12 = -k03 * s5 + k23 * s2 - m33 * s1;
    const T a13 = k02 * s5 - m22 * s2 + k23 * s1;
    const T a22 = k03 * s4 - k13 * s2 + m33 * s0;
    const T a23 = -k02 * s4 + k12 * s2 - k23 * s0;
    const T a33 = k02 * s3 - k12 * s1 + m22 * s0;

    // column with the largest |diagonal| (q_j^2 >= 1/4 there)
    T q0 = a00, q1 = a01, q2 = a02, q3 = a03, best = tabs(a00);
    if (tabs(a11) > best) { best = tabs(a11); q0 = a01; q1 = a11; q2 = a12; q3 = a13; }
    if (tabs(a22) > best) { best = tabs(a22); q0 = a02; q1 = a12; q2 = a22; q3 = a23; }
    if (tabs(a33) > best) { best = tabs(a33); q0 = a03; q1 = a13; q2 = a23; q3 = a33; }
    const T n2 = q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3;
    if (!(n2 > tiny) || !(n2 < huge)) { // K - lam I numerically zero: degenerate input
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? (RT)1 : (RT)0;
        return;
    }
    // 1/n2: fp32 reciprocal seed + one Newton step in fp64 (relative error ~1e-14)
    T inv = (T)fast_rcp((float)n2);
    inv = inv * ((T)2 - n2 * inv);
    if (sizeof(RT) == 8) inv = inv * ((T)2 - n2 * inv);   // rotation wanted in double: one more step (1e-14 -> rounding)
    const T ww = q0 * q0 * inv, xx = q1 * q1 * inv, yy = q2 * q2 * inv, zz = q3 * q3 * inv;
    const T wx = q0 * q1 * inv, wy = q0 * q2 * inv, wz = q0 * q3 * inv;
    const T xy = q1 * q2 * inv, xz = q1 * q3 * inv, yz = q2 * q3 * inv;
    // Q (column convention, maps frame -> reference); R = Q^T for row vectors
    R[0] = (RT)(ww + xx - yy - zz);
    R[1] = (RT)((T)2 * (xy + wz));
    R[2] = (RT)((T)2 * (xz - wy));
    R[3] = (RT)((T)2 * (xy - wz));
    R[4] = (RT)(ww - xx + yy - zz);
    R[5] = (RT)((T)2 * (yz + wx));
    R[6] = (RT)((T)2 * (xz + wy));
    R[7] = (RT)((T)2 * (yz - wx));
    R[8] = (RT)(ww - xx - yy + zz);
}

MOLANN_HD void kabsch_rotation(const double (&H)[9], double e0, float (&R)[9]) { kabsch_rotation_t<double>(H, e0, R); }
MOLANN_HD void kabsch_rotation_f32(const float (&H)[9], float e0, float (&R)[9]) { kabsch_rotation_t<float>(H, e0, R); }

// y = p . R  (row vector times row-major R)
MOLANN_HD V3 rotate(V3 p, const float (&R)[9]) {
    return v3(fmaf(p.z, R[6], fmaf(p.y, R[3], p.x * R[0])), fmaf(p.z, R[7], fmaf(p.y, R[4], p.x * R[1])),
              fmaf(p.z, R[8], fmaf(p.y, R[5], p.x * R[2])));
}

// The atoms of one item as the feature sees them in the ALIGNED frame y = ((p - c0) - dl) R (ann.py:197, 565).  A position
// item needs y itself.  Bond / angle / dihedral items are translation invariant: they are evaluated about the item's second
// atom, y_k - y_1 = (p_k - p_1) R, so the short vectors between neighbouring atoms are formed from the INPUT coordinates
// (exact up to the rounding of a vector of a few Angstrom) rather than from aligned coordinates that each carry the
// rounding of their distance to the centroid - 1e-5 A at 100 A, which is what a 5000-atom frame's outer atoms have, and
// what an ill-conditioned dihedral then amplifies.  Same values in exact arithmetic; used by the large-frame forward kernels and,
// for the atoms handed to eval_item_backward, by every backward kernel.
MOLANN_HD void align_item_atoms(int type, V3& p0, V3& p1, V3& p2, V3& p3, V3 c0, V3 dl, const float (&R)[9]) {
    if (type == IT_POSITION) {
        p0 = rotate((p0 - c0) - dl, R);
        return;
    }
    p0 = rotate(p0 - p1, R);
    p2 = rotate(p2 - p1, R);
    p3 = rotate(p3 - p1, R);
    p1 = v3(0.f, 0.f, 0.f);
}

// =================================================================================================
// float64 instantiation of the forward (the reference follows x.dtype: `model.double()(x.double())`, ann.py:187-197,
// 323-354).  Plain double arithmetic with libm - no fast approximations: the bar is 1e-10 against the reference's
// own float64 run.
// =================================================================================================
struct V3d {
    double x, y, z;
};
MOLANN_HD V3d v3d(double x, double y, double z) { V3d r; r.x = x; r.y = y; r.z = z; return r; }
MOLANN_HD V3d operator-(V3d a, V3d b) { return v3d(a.x - b.x, a.y - b.y, a.z - b.z); }
MOLANN_HD double dot(V3d a, V3d b) { return fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)); }
MOLANN_HD V3d cross(V3d a, V3d b) {
    return v3d(fma(a.y, b.z, -(a.z * b.y)), fma(a.z, b.x, -(a.x * b.z)), fma(a.x, b.y, -(a.y * b.x)));
}
MOLANN_HD V3d rotate(V3d p, const double (&R)[9]) {
    return v3d(fma(p.z, R[6], fma(p.y, R[3], p.x * R[0])), fma(p.z, R[7], fma(p.y, R[4], p.x * R[1])),
               fma(p.z, R[8], fma(p.y, R[5], p.x * R[2])));
}
// eval_item in double (same item types, same column order)
MOLANN_HD int eval_item_f64(int type, V3d a0, V3d a1, V3d a2, V3d a3, double (&out)[3]) {
    switch (type) {
    case IT_ANGLE_COS:
    case IT_ANGLE_VAL: {
        const V3d r21 = a0 - a1, r23 = a2 - a1;
        if (type == IT_ANGLE_VAL) {   // atan2(|u x v|, u.v), as eval_item
            const V3d w = cross(r21, r23);
            out[0] = atan2(sqrt(dot(w, w)), dot(r21, r23));
            return 1;
        }
        out[0] = dot(r21, r23) / (sqrt(dot(r21, r21)) * sqrt(dot(r23, r23)));   // ann.py:324-328, no clamp
        return 1;
    }
    case IT_BOND: {
        const V3d r = a1 - a0;
        out[0] = sqrt(dot(r, r));
        return 1;
    }
    case IT_DIHEDRAL_CS:
    case IT_DIHEDRAL_VAL: {
        const V3d r12 = a1 - a0, r23 = a2 - a1, r34 = a3 - a2;
        const V3d n1 = cross(r12, r23), n2 = cross(r23, r34);
        const double c = dot(n1, n2), sn = dot(n1, r34) * sqrt(dot(r23, r23));
        if (type == IT_DIHEDRAL_VAL) { out[0] = atan2(sn, c); return 1; }
        const double radius = sqrt(fma(c, c, sn * sn));                              // ann.py:346
        out[0] = c / radius;
        out[1] = sn / radius;
        return 2;
    }
    default:
        out[0] = a0.x; out[1] = a0.y; out[2] = a0.z;
        return 3;
    }
}
MOLANN_HD double apply_activation_f64(int act, double v) {
    switch (act) {
    case 0: return tanh(v);
    case 1: return v > 0.0 ? v : (v != v ? v : 0.0);
    case 2: return 1.0 / (1.0 + exp(-v));
    case 3: return v;
    case 4: return v > 0.0 ? v : expm1(v);
    case 5: return v / (1.0 + exp(-v));
    case 6: return v > 20.0 ? v : log1p(exp(v));
    case 7: return v > 0.0 ? v : 0.01 * v;
    case 8: return 0.5 * v * (1.0 + erf(v * 0.70710678118654752));
    default: return v;
    }
}

// =================================================================================================
// reverse mode (backward of the path; the reference relies on torch autograd for all of it)
// =================================================================================================
MOLANN_HD V3 operator*(float s, V3 a) { return v3(s * a.x, s * a.y, s * a.z); }
MOLANN_HD void axpy(V3& acc, float s, V3 a) { acc.x = fmaf(s, a.x, acc.x); acc.y = fmaf(s, a.y, acc.y); acc.z = fmaf(s, a.z, acc.z); }

// Gradient of one feature item with respect to its (aligned) atoms: g[] is dL/d(output columns of the item),
// ga0..ga3 are ACCUMULATED into.  Mirrors eval_item; formulas are the reverse-mode of ann.py:323-354.
MOLANN_HD void eval_item_backward(int type, V3 a0, V3 a1, V3 a2, V3 a3, const float (&g)[3], V3& ga0, V3& ga1, V3& ga2,
                                  V3& ga3) {
    switch (type) {
    case IT_BOND: {
        const V3 r = a1 - a0;
        const float d2 = dot(r, r);
        const float inv = d2 == 0.0f ? 0.0f : fast_rsq(d2); // |r| = 0: subgradient 0; a |r| that is not finite stays so
        axpy(ga1, g[0] * inv, r);
        axpy(ga0, -g[0] * inv, r);
        return;
    }
    case IT_ANGLE_COS:
    case IT_ANGLE_VAL: {
        const V3 u = a0 - a1, v = a2 - a1;
        const float uu = dot(u, u), vv = dot(v, v), uv = dot(u, v);
        if (type == IT_ANGLE_VAL) {
            // d theta/du = u x w / (|u|^2 |w|), d theta/dv = w x v / (|v|^2 |w|), w = u x v: each of length 1/|arm| by construction
            // (u x w is perpendicular to both), at any angle; the only rounding that grows is w's own, eps / sin(theta).  The
            // chain rule through acos, -dc / sqrt(1 - c^2), cancels twice (eps / sin^2) and, once c rounds to +-1, needs a clamp
            // that turns the pole into a finite gradient of 1e15.  Here w = 0 gives 0 * inf = NaN, as the reference's autograd does.
            const V3 w = cross(u, v);
            const float gw = g[0] * fast_rsq(dot(w, w));
            const V3 gu = (gw * fast_rcp(uu)) * cross(u, w), gv = (gw * fast_rcp(vv)) * cross(w, v);
            ga0 = ga0 + gu;
            ga2 = ga2 + gv;
            ga1 = ga1 - (gu + gv);
            return;
        }
        const float inv_uv = fast_rsq(uu * vv); // 1 / (|u||v|)
        const float c = uv * inv_uv;
        const float gc = g[0];
        // dc/du = v/(|u||v|) - c u/|u|^2 ,  dc/dv = u/(|u||v|) - c v/|v|^2
        V3 gu = v3(0.f, 0.f, 0.f), gv = v3(0.f, 0.f, 0.f);
        axpy(gu, gc * inv_uv, v); axpy(gu, -gc * c * fast_rcp(uu), u);
        axpy(gv, gc * inv_uv, u); axpy(gv, -gc * c * fast_rcp(vv), v);
        ga0 = ga0 + gu;
        ga2 = ga2 + gv;
        ga1 = ga1 - (gu + gv);
        return;
    }
    case IT_DIHEDRAL_CS:
    case IT_DIHEDRAL_VAL: {
        const V3 r12 = a1 - a0, r23 = a2 - a1, r34 = a3 - a2;
        const V3 n1 = cross(r12, r23), n2 = cross(r23, r34);
        const float L2 = dot(r23, r23);
        const float L = fast_sqrt(L2);
        const float n1r34 = dot(n1, r34);
        const float C = dot(n1, n2), S = n1r34 * L;
        const float rad2 = fmaf(C, C, S * S);
        float gC, gS;
        if (type == IT_DIHEDRAL_CS) { // outputs (C, S) / rad
            const float inv_rad = fast_rsq(rad2);
            const float proj = (g[0] * C + g[1] * S) * inv_rad * inv_rad * inv_rad;
            gC = g[0] * inv_rad - proj * C;
            gS = g[1] * inv_rad - proj * S;
        } else { // atan2(S, C): d phi = (C dS - S dC) / rad^2
            const float inv_rad2 = fast_rcp(rad2);
            gC = -g[0] * S * inv_rad2;
            gS = g[0] * C * inv_rad2;
        }
        // C = n1.n2 ; S = (n1.r34) L
        V3 gn1 = gC * n2; axpy(gn1, gS * L, r34);
        const V3 gn2 = gC * n1;
        V3 gr34 = (gS * L) * n1;
        V3 gr23 = (L > 0.0f ? gS * n1r34 * fast_rcp(L) : 0.0f) * r23;
        // n1 = r12 x r23 ; n2 = r23 x r34      (n = a x b  =>  ga = b x gn , gb = gn x a)
        const V3 gr12 = cross(r23, gn1);
        gr23 = gr23 + cross(gn1, r12) + cross(r34, gn2);
        gr34 = gr34 + cross(gn2, r23);
        ga0 = ga0 - gr12;
        ga1 = ga1 + (gr12 - gr23);
        ga2 = ga2 + (gr23 - gr34);
        ga3 = ga3 + gr34;
        return;
    }
    default: // IT_POSITION
        ga0 = ga0 + v3(g[0], g[1], g[2]);
        return;
    }
}

// Derivative of the activation expressed with its OUTPUT h (and input z where the output is not enough).
MOLANN_HD float act_derivative(int act, float z, float h) {
    switch (act) {
    case 0: return fmaf(-h, h, 1.0f);          // tanh' = 1 - tanh^2
    case 1: return z > 0.0f ? 1.0f : 0.0f;     // ReLU
    case 2: return h * (1.0f - h);             // sigmoid' = s (1 - s)
    case 3: return 1.0f;                       // identity
    case 5: { const float s = act_sigmoid(z); return s * fmaf(z, 1.0f - s, 1.0f); } // SiLU' = s (1 + z (1 - s))
    case 7: return z > 0.0f ? 1.0f : 0.01f;    // LeakyReLU
    default: return 1.0f;
    }
}

// Derivative of apply_activation_f64 from its INPUT z (the float64 head keeps its pre-activations), all nine codes.
MOLANN_HD double act_derivative_f64(int act, double z) {
    switch (act) {
    case 0: { const double t = tanh(z); return fma(-t, t, 1.0); }
    case 1: return z > 0.0 ? 1.0 : 0.0;                    // torch's convention at 0
    case 2: { const double s = 1.0 / (1.0 + exp(-z)); return s * (1.0 - s); }
    case 3: return 1.0;
    case 4: return z > 0.0 ? 1.0 : exp(z);                 // ELU(alpha=1)
    case 5: { const double s = 1.0 / (1.0 + exp(-z)); return s * fma(z, 1.0 - s, 1.0); }   // SiLU' = s (1 + z (1 - s))
    case 6: return z > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-z)); // Softplus(beta=1, threshold=20)
    case 7: return z > 0.0 ? 1.0 : 0.01;
    case 8: return fma(z * 0.39894228040143267794, exp(-0.5 * z * z), 0.5 * (1.0 + erf(z * 0.70710678118654752)));   // Phi(z) + z phi(z)
    default: return 1.0;
    }
}

// One output's term of a harmonic restraint E = 1/2 sum_k kappa_k d_k^2 (umbrella sampling, steered MD, the string method's replicas):
// d = y - z, wrapped into [-P/2, P/2] where the output is periodic (period > 0; rint: ties to even), moved to the wall of a flat-bottomed
// well where flat > 0 (d = 0 inside |d| <= flat, copysign(|d| - flat, d) outside; a NaN d stays NaN).  Returns 1/2 kappa d^2 and
// dy = kappa d, the term's derivative with respect to y; kappa may have any sign.  Nothing is contracted: every operation rounds once,
// so with no period and no flat dy is the rounded product of kappa and the rounded y - z, on the host and on the device.
MOLANN_HD double restraint_term_f64(double y, double z, double kappa, double period, double flat, double& dy) {
#pragma clang fp contract(off)
    double d = y - z;
    if (period > 0.0) {
        const double turns = rint(d / period);
        const double whole = period * turns;
        d = d - whole;
    }
    if (flat > 0.0) {
        const double a = fabs(d) - flat;
        if (a > 0.0) d = copysign(a, d);
        else if (a <= 0.0) d = 0.0;     // neither holds for a NaN, which stays
    }
    dy = kappa * d;
    return 0.5 * dy * d;
}

// One Gaussian hill of a metadynamics bias V(y) = sum_h w_h exp(-1/2 sum_k ((y_k - c_hk) / sigma_hk)^2) on d <= HILLS_MAX_D outputs:
// d_k = y_k - c_k, wrapped like restraint_term_f64's where period_k > 0 (period may be null), s_k = d_k / sigma_k formed as d_k times
// the rounded 1 / sigma_k (one division per column, not two), q = 1/2 sum_k s_k^2 with k ascending, g = w exp(-q).  Returns g and adds
// g s_k / sigma_k to acc[k]: the bias is the sum of the returned values, dV/dy_k the NEGATIVE of acc[k].  w may have any sign; a far
// hill's exp underflows to 0 and adds exact zeros; a NaN in y or c makes g and every acc[k] NaN.  Nothing is contracted, so the host
// and the device round alike up to exp.  acc is a fixed array indexed by constants only: registers on the device.  Where one row of
// widths serves every hill (`shared`) the caller forms the 1 / sigma_k once, with hill_inverse_widths_f64, and sigma is not read here:
// the same rounded values, so a shared row and the same row repeated per hill give the same bits.
constexpr int HILLS_MAX_D = 8;
MOLANN_HD void hill_inverse_widths_f64(const double* sigma, int d, double (&inv)[HILLS_MAX_D]) {
#pragma unroll
    for (int k = 0; k < HILLS_MAX_D; ++k) inv[k] = k < d ? 1.0 / sigma[k] : 0.0;
}
MOLANN_HD double hill_term_f64(const double* y, const double* c, const double* sigma, const double (&inv_shared)[HILLS_MAX_D], bool shared,
                               const double* period, double w, int d, double (&acc)[HILLS_MAX_D]) {
#pragma clang fp contract(off)
    double t[HILLS_MAX_D];
    double q = 0.0;
#pragma unroll
    for (int k = 0; k < HILLS_MAX_D; ++k) {
        t[k] = 0.0;
        if (k < d) {
            double dk = y[k] - c[k];
            const double P = period ? period[k] : 0.0;
            if (P > 0.0) {
                const double turns = rint(dk / P);
                const double whole = P * turns;
                dk = dk - whole;
            }
            const double inv = shared ? inv_shared[k] : 1.0 / sigma[k];
            const double s = dk * inv;
            q = q + s * s;
            t[k] = s * inv;
        }
    }
    const double g = w * exp(-(0.5 * q));
#pragma unroll
    for (int k = 0; k < HILLS_MAX_D; ++k)
        if (k < d) acc[k] = acc[k] + g * t[k];
    return g;
}

// One kernel of an OPES bias V(y) = scale log(P(y) / norm + epsilon), P(y) = sum_h w_h (exp(-q_h / 2) - exp(-cutoff^2 / 2)) over the
// kernels with q_h < cutoff^2, q_h = sum_k (d_hk / sigma_hk)^2, on d <= HILLS_MAX_D outputs.  d_k, its wrap by period_k, 1 / sigma_k,
// s_k = d_k (1 / sigma_k) and the ascending-k sum of s_k^2 are hill_term_f64's, operation for operation (so are `shared` and
// hill_inverse_widths_f64); here q is that sum, not its half.  c2 = cutoff^2 and c0 = exp(-(0.5 c2)) come from the caller, once per
// frame (opes_cutoff_f64).  A kernel with q >= c2 is dropped: it returns 0 and adds nothing, so a table with it and without it gives
// the same bits.  Otherwise e = exp(-(0.5 q)): returns w (e - c0) and adds (w e) s_k / sigma_k to acc[k], so dP/dy_k is the NEGATIVE of
// acc[k].  The test is q >= c2 and not !(q < c2): a NaN q fails it, reaches exp and makes the return and every acc[k] NaN.  cutoff =
// +inf: c2 = +inf, c0 = 0, nothing is dropped.  The exp of a dropped kernel is computed and its results not taken (a select; measured
// against a branch around the exp, which is no faster: the lanes of a wave hold different kernels and seldom all drop theirs, see
// DESIGN.md); either form gives the same values.  Nothing is contracted, so the host and the device round alike up to exp.
MOLANN_HD void opes_cutoff_f64(double cutoff, double& c2, double& c0) {
#pragma clang fp contract(off)
    c2 = cutoff * cutoff;
    c0 = exp(-(0.5 * c2));
}
MOLANN_HD double opes_term_f64(const double* y, const double* c, const double* sigma, const double (&inv_shared)[HILLS_MAX_D], bool shared,
                               const double* period, double w, double c2, double c0, int d, double (&acc)[HILLS_MAX_D]) {
#pragma clang fp contract(off)
    double t[HILLS_MAX_D];
    double q = 0.0;
#pragma unroll
    for (int k = 0; k < HILLS_MAX_D; ++k) {
        t[k] = 0.0;
        if (k < d) {
            double dk = y[k] - c[k];
            const double P = period ? period[k] : 0.0;
            if (P > 0.0) {
                const double turns = rint(dk / P);
                const double whole = P * turns;
                dk = dk - whole;
            }
            const double inv = shared ? inv_shared[k] : 1.0 / sigma[k];
            const double s = dk * inv;
            q = q + s * s;
            t[k] = s * inv;
        }
    }
    const bool drop = q >= c2;
    const double e = exp(-(0.5 * q));
    const double g = w * e;
#pragma unroll
    for (int k = 0; k < HILLS_MAX_D; ++k)
        if (k < d) acc[k] = drop ? acc[k] : acc[k] + g * t[k];
    return drop ? 0.0 : w * (e - c0);
}

// The transform of an OPES bias, once per frame after the sums: u = P / norm + epsilon, V = scale log(u), f = scale / (norm u) and
// cot[k] = dV/dy_k = -(f acc[k]) for the acc opes_term_f64 summed.  P = 0 and acc = 0 (no kernel yet, or every kernel past the
// cutoff): V = scale log(epsilon), cot exactly 0 (-(f 0) is -0.0, which compares equal).  u <= 0 needs negative weights, which are
// the caller's to avoid: log and the division give NaN or +-inf for that frame.  Nothing is contracted.
MOLANN_HD double opes_transform_f64(double P, const double (&acc)[HILLS_MAX_D], double scale, double norm, double epsilon, int d,
                                    double (&cot)[HILLS_MAX_D]) {
#pragma clang fp contract(off)
    const double u = P / norm + epsilon;
    const double f = scale / (norm * u);
#pragma unroll
    for (int k = 0; k < HILLS_MAX_D; ++k) cot[k] = k < d ? -(f * acc[k]) : 0.0;
    return scale * log(u);
}

// The per-kernel arithmetic of an OPES deposit (opes_deposit_f64_kernel and its host twin): compressing a new kernel into the table and
// keeping S = sum_i sum_j h_j K_j(c_i) over the live kernels, the sum the normalisation Z is formed from.  Nothing is contracted.
//
// opes_merge_distance_f64: q = sum_k (wrap(a_k - c_k) / sigma_k)^2 of a candidate centre `a` from the table kernel (c, sigma), in the
// table kernel's widths: opes_term_f64's d_k, wrap, 1 / sigma_k, product and ascending-k sum, operation for operation, and no exp, so
// the host and the device get the same bits and take the same decisions.
MOLANN_HD double opes_merge_distance_f64(const double* a, const double* c, const double* sigma, const double* period, int d) {
#pragma clang fp contract(off)
    double q = 0.0;
#pragma unroll
    for (int k = 0; k < HILLS_MAX_D; ++k) {
        if (k < d) {
            double dk = a[k] - c[k];
            const double P = period ? period[k] : 0.0;
            if (P > 0.0) {
                const double turns = rint(dk / P);
                const double whole = P * turns;
                dk = dk - whole;
            }
            const double inv = 1.0 / sigma[k];
            const double s = dk * inv;
            q = q + s * s;
        }
    }
    return q;
}

// opes_merge_f64: the giver (cg, sg, hg) merges into the taker (ct, st, ht): h' = ht + hg, delta_k = wrap(cg_k - ct_k),
// c'_k = ct_k + (hg / h') delta_k and sigma'_k^2 = (ht st_k^2 + hg sg_k^2) / h' + (ht hg / h'^2) delta_k^2 - the weight, mean and variance
// of the two kernels' mixture, the mean taken along the shorter way round a periodic output (c' is not wrapped back: every reader wraps
// differences).  Returns h'; co and so may be either kernel's arrays (column k is read before it is written).  Only +, -, *, /, rint and
// sqrt: the host and the device round alike up to sqrt.
MOLANN_HD double opes_merge_f64(const double* ct, const double* st, double ht, const double* cg, const double* sg, double hg, const double* period,
                                int d, double* co, double* so) {
#pragma clang fp contract(off)
    const double h = ht + hg;
    const double wg = hg / h;
    const double wtg = (ht * hg) / (h * h);
#pragma unroll
    for (int k = 0; k < HILLS_MAX_D; ++k) {
        if (k < d) {
            double dk = cg[k] - ct[k];
            const double P = period ? period[k] : 0.0;
            if (P > 0.0) {
                const double turns = rint(dk / P);
                const double whole = P * turns;
                dk = dk - whole;
            }
            const double var = (ht * (st[k] * st[k]) + hg * (sg[k] * sg[k])) / h + wtg * (dk * dk);
            co[k] = ct[k] + wg * dk;
            so[k] = sqrt(var);
        }
    }
    return h;
}

// opes_pair_term_f64: what the kernels e and i add to S together, h_e K_e(c_i) + h_i K_i(c_e), each half opes_term_f64 with its result
// taken and its acc ignored; inv_e is hill_inverse_widths_f64 of e's widths, formed once per walk (the same rounded values as 1 / sigma
// per term).  A kernel's own term is h (1 - c0): opes_self_term_f64.
MOLANN_HD double opes_pair_term_f64(const double* ce, const double* se, const double (&inv_e)[HILLS_MAX_D], double he, const double* ci,
                                    const double* si, double hi, const double* period, double c2, double c0, int d) {
#pragma clang fp contract(off)
    double ignored[HILLS_MAX_D] = {0., 0., 0., 0., 0., 0., 0., 0.};
    const double at_i = opes_term_f64(ci, ce, se, inv_e, true, period, he, c2, c0, d, ignored);
    const double at_e = opes_term_f64(ce, ci, si, inv_e, false, period, hi, c2, c0, d, ignored);
    return at_i + at_e;
}
MOLANN_HD double opes_self_term_f64(double h, double c0) {
#pragma clang fp contract(off)
    return h * (1.0 - c0);
}

// a new kernel is taken when every value is finite, every width > 0 and the height > 0 (a NaN fails every comparison)
MOLANN_HD bool opes_kernel_valid_f64(const double* c, const double* sigma, double h, int d) {
    bool ok = h > 0.0 && h <= 1.7976931348623157e308;
#pragma unroll
    for (int k = 0; k < HILLS_MAX_D; ++k)
        if (k < d) ok = ok && fabs(c[k]) <= 1.7976931348623157e308 && sigma[k] > 0.0 && sigma[k] <= 1.7976931348623157e308;
    return ok;
}

// the live count of a deposit's state: an exact integer in a double, held to [0, capacity] whatever the bits (a NaN gives 0)
MOLANN_HD long opes_live_count_f64(double n, long capacity) {
    return n >= (double)capacity ? capacity : n >= 1.0 ? (long)n : 0;
}

// The deposit itself, one copy for the device and the host: `ex` gives the table (load_new, load, store, move), the search
// (nearest: the live kernel with the smallest opes_merge_distance_f64 from a centre, then the smallest slot, one slot left out; false
// where there is none) and the walk (pair_sum: sum of opes_pair_term_f64 over the live kernels, two slots left out, in its fixed
// order); every thread of the device's block runs these steps on the same values and takes the same decisions.  Per new kernel, in
// order: refused unless opes_kernel_valid_f64; then, as the giver g (not in the table yet: slot -1), while a live kernel t other than g
// lies within the threshold (q < threshold^2, strict): S loses g's terms (where g is in the table) and t's, t takes g by
// opes_merge_f64 and stays in its slot, S gains the merged kernel's terms, g's slot is filled by the last live kernel (which may be t),
// and the merged kernel is the next giver.  Every round but a new kernel's first removes a kernel, so the chain ends.  A new kernel
// that met nobody is appended while there is room and refused otherwise.  n, S, merges and refused are the state's four values.
template <class Ex>
MOLANN_HD void opes_deposit_steps_f64(Ex& ex, long capacity, int d, const double* period, long n_new, double threshold, double cutoff, long& n,
                                      double& S, double& merges, double& refused) {
#pragma clang fp contract(off)
    double c2, c0;
    opes_cutoff_f64(cutoff, c2, c0);
    const double thr2 = threshold * threshold;
    for (long a = 0; a < n_new; ++a) {
        double cg[HILLS_MAX_D], sg[HILLS_MAX_D], hg;
        ex.load_new(a, cg, sg, hg);
        if (!opes_kernel_valid_f64(cg, sg, hg, d)) {
            refused = refused + 1.0;
            continue;
        }
        long g = -1;
        for (;;) {
            double q = 0.0;
            long t = -1;
            if (!(threshold > 0.0 && ex.nearest(cg, n, g, q, t) && q < thr2)) break;
            double ct[HILLS_MAX_D], st[HILLS_MAX_D], ht;
            ex.load(t, ct, st, ht);
            if (g >= 0) S = S - (ex.pair_sum(cg, sg, hg, n, g, -1, c2, c0) + opes_self_term_f64(hg, c0));   // remove g; t is still live
            S = S - (ex.pair_sum(ct, st, ht, n, t, g, c2, c0) + opes_self_term_f64(ht, c0));                 // remove t
            hg = opes_merge_f64(ct, st, ht, cg, sg, hg, period, d, cg, sg);
            S = S + (ex.pair_sum(cg, sg, hg, n, t, g, c2, c0) + opes_self_term_f64(hg, c0));                 // add the merged kernel
            ex.store(t, cg, sg, hg);
            merges = merges + 1.0;
            if (g >= 0) {
                if (g != n - 1) ex.move(n - 1, g);
                if (t == n - 1) t = g;
                n -= 1;
            }
            g = t;
        }
        if (g >= 0) continue;
        if (n < capacity) {
            S = S + (ex.pair_sum(cg, sg, hg, n, -1, -1, c2, c0) + opes_self_term_f64(hg, c0));
            ex.store(n, cg, sg, hg);
            n += 1;
        } else {
            refused = refused + 1.0;
        }
    }
}

// The scalar arithmetic of a whole OPES step (opes_step_f64_kernel and its host twin; OPES_METAD's update with a fixed sigma0, not the
// explore variant), on run[8] = (counter, sum_w, sum_w2, neff, sigma_scale, rct, 0, 0).  Nothing is contracted, so the host and the
// device round alike up to exp, log and pow.
//
// opes_table_norm_f64: the `norm` of opes_transform_f64 from a table's state, Z kde_norm = S / n (Z = S / (n kde_norm)).  n >= 1.
MOLANN_HD double opes_table_norm_f64(double S, long n) {
    return S / (double)n;
}

// opes_walker_weight_f64: w = exp(beta V) of one walker, and whether the walker counts: V, w and every y_k finite and w > 0 (a NaN
// fails every comparison; an exp that overflows, or underflows to 0, fails too).
MOLANN_HD bool opes_walker_weight_f64(double beta, double V, const double* y, int d, double& w) {
#pragma clang fp contract(off)
    w = exp(beta * V);
    bool ok = fabs(V) <= 1.7976931348623157e308 && w > 0.0 && w <= 1.7976931348623157e308;
#pragma unroll
    for (int k = 0; k < HILLS_MAX_D; ++k)
        if (k < d) ok = ok && fabs(y[k]) <= 1.7976931348623157e308;
    return ok;
}

// one valid walker into a thread's three partial sums
MOLANN_HD void opes_walker_add_f64(double w, double& count, double& sum_w, double& sum_w2) {
#pragma clang fp contract(off)
    const double w2 = w * w;
    count = count + 1.0;
    sum_w = sum_w + w;
    sum_w2 = sum_w2 + w2;
}

// opes_run_scalars_f64: neff = (1 + sum_w)^2 / (1 + sum_w2), rct = log(sum_w / counter) / beta (0 while counter == 0) and the
// bandwidth rescaling sigma_scale = (neff (d + 2) / 4)^(-1 / (d + 4)) (Silverman's rule on the effective sample size; 1 with
// `fixed_sigma`), from the sums after this step's walkers.
MOLANN_HD void opes_run_scalars_f64(double counter, double sum_w, double sum_w2, double beta, int d, int fixed_sigma, double& neff,
                                    double& sigma_scale, double& rct) {
#pragma clang fp contract(off)
    const double a = 1.0 + sum_w;
    neff = (a * a) / (1.0 + sum_w2);
    rct = counter > 0.0 ? log(sum_w / counter) / beta : 0.0;
    const double dd = (double)d;
    sigma_scale = fixed_sigma ? 1.0 : pow((neff * (dd + 2.0)) / 4.0, -1.0 / (dd + 4.0));
}

// opes_step_widths_f64: the widths of this step's kernels, sigma_k = sigma0_k sigma_scale raised to sigma_min_k where sigma_min is
// given (sigma_k < sigma_min_k: a NaN stays), the same for every walker.  Returns prod_k (sigma0_k / sigma_k), k ascending: what a
// kernel's height gains where its width was held up, so that its integral stays its weight.
MOLANN_HD double opes_step_widths_f64(const double* sigma0, const double* sigma_min, double sigma_scale, int d, double (&sigma)[HILLS_MAX_D]) {
#pragma clang fp contract(off)
    double ratio = 1.0;
#pragma unroll
    for (int k = 0; k < HILLS_MAX_D; ++k) {
        sigma[k] = 1.0;
        if (k < d) {
            double s = sigma0[k] * sigma_scale;
            if (sigma_min && s < sigma_min[k]) s = sigma_min[k];
            sigma[k] = s;
            ratio = ratio * (sigma0[k] / s);
        }
    }
    return ratio;
}

// the height of walker a's kernel: w_a ratio, or NaN for a walker that does not count - opes_kernel_valid_f64 refuses it
MOLANN_HD double opes_walker_height_f64(double beta, double V, const double* y, int d, double ratio) {
#pragma clang fp contract(off)
    double w;
    const bool ok = opes_walker_weight_f64(beta, V, y, d, w);
    return ok ? w * ratio : __builtin_nan("");
}

// The step itself, one copy for the device and the host: `ex` is a deposit executor (opes_deposit_steps_f64) that also gives the
// step's three sums over the valid walkers in their fixed order (walker_sums) and whose load_new(a) yields (y[a], ex.step_sigma,
// opes_walker_height_f64 with ex.ratio).  In order: the sums join run[0..2]; the scalars; the widths; the deposit of the W kernels.
template <class Ex>
MOLANN_HD void opes_step_steps_f64(Ex& ex, long capacity, int d, const double* period, long n_walkers, double threshold, double cutoff,
                                   double beta, int fixed_sigma, const double* sigma0, const double* sigma_min, long& n, double& S,
                                   double& merges, double& refused, double (&run)[8]) {
#pragma clang fp contract(off)
    double count, sum_w, sum_w2;
    ex.walker_sums(n_walkers, count, sum_w, sum_w2);
    run[0] = run[0] + count;
    run[1] = run[1] + sum_w;
    run[2] = run[2] + sum_w2;
    opes_run_scalars_f64(run[0], run[1], run[2], beta, d, fixed_sigma, run[3], run[4], run[5]);
    run[6] = 0.0;
    run[7] = 0.0;
    ex.ratio = opes_step_widths_f64(sigma0, sigma_min, run[4], d, ex.step_sigma);
    opes_deposit_steps_f64(ex, capacity, d, period, n_walkers, threshold, cutoff, n, S, merges, refused);
}

// A bias tabulated on a regular grid over d <= GRID_MAX_D outputs, interpolated by cubic convolution (Catmull-Rom): V(y) = sum over the
// 4^d stencil points of T[idx_0 j0, ...] prod_k a_k jk, dV/dy_k the same sum with b_k jk in place of a_k jk.  grid_axis_f64 is one
// axis' step: u = (y - lower) / h; periodic: u <- u - n floor(u / n), i = floor(u) held in [0, n - 1], idx_j = (i - 1 + j) mod n;
// not periodic: s = 1 inside [0, n - 1], else s = 0 and u is clamped to it, i = floor(u) held in [0, n - 2], idx_j = i - 1 + j clamped
// to [0, n - 1] (the edge's value repeats); t = u - i, a_j = w_j(t), b_j = s w'_j(t) / h.  Outside a non-periodic range V is the edge's
// value and that axis' derivative exactly 0: the derivative jumps at the range's ends.  Every idx lies in [0, n - 1] for every bit
// pattern of y: the cell index is formed in double, held to its range by comparisons that a NaN fails towards 0, and only then
// converted; a u that is not finite takes cell 0 and a NaN t, so the frame's bias and derivatives are NaN.  Nothing is contracted.
constexpr int GRID_MAX_D = 3;
MOLANN_HD void grid_axis_f64(double y, long n, double lower, double h, bool periodic, long (&idx)[4], double (&a)[4], double (&b)[4]) {
#pragma clang fp contract(off)
    const double nd = (double)n;
    double u = (y - lower) / h;
    double s = 1.0, fi = 0.0, t;
    if (!(fabs(u) <= 1.7976931348623157e308)) {    // NaN, +-inf
        t = u - u;                                 // NaN
    } else if (periodic) {
        u = u - nd * floor(u / nd);
        fi = floor(u);
        fi = fi >= 0.0 ? fi : 0.0;
        fi = fi <= nd - 1.0 ? fi : nd - 1.0;
        t = u - fi;
    } else {
        if (!(u >= 0.0)) { s = 0.0; u = 0.0; }
        if (!(u <= nd - 1.0)) { s = 0.0; u = nd - 1.0; }
        fi = floor(u);
        fi = fi <= nd - 2.0 ? fi : nd - 2.0;
        t = u - fi;
    }
    const long i = (long)fi;    // an integer in [0, n - 1]
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        long q = i - 1 + j;
        if (periodic) q = q < 0 ? q + n : q >= n ? q - n : q;
        else q = q < 0 ? 0 : q > n - 1 ? n - 1 : q;
        idx[j] = q;
    }
    const double t2 = t * t;
    a[0] = ((-t + 2.0) * t - 1.0) * t / 2.0;
    a[1] = ((3.0 * t - 5.0) * t2 + 2.0) / 2.0;
    a[2] = ((-3.0 * t + 4.0) * t + 1.0) * t / 2.0;
    a[3] = (t - 1.0) * t2 / 2.0;
    const double sh = s / h;
    b[0] = sh * ((-3.0 * t2 + 4.0 * t - 1.0) / 2.0);
    b[1] = sh * ((9.0 * t2 - 10.0 * t) / 2.0);
    b[2] = sh * ((-9.0 * t2 + 8.0 * t + 1.0) / 2.0);
    b[3] = sh * ((3.0 * t2 - 2.0 * t) / 2.0);
}

// entry j of a 4-array by comparisons, so that an array indexed by a value known only at run time stays in registers
template <typename T>
MOLANN_HD T grid_pick(const T (&v)[4], int j) { return j == 0 ? v[0] : j == 1 ? v[1] : j == 2 ? v[2] : v[3]; }

// Stencil point p of 4^d (j_k = (p >> 2k) & 3) of the bias above: returns T[...] prod_k a_k jk and stores T[...] b_k jk prod_{m != k} a_m jm
// in term[k] (0 for k >= d).  The table is row-major with output 0 slowest; the offset is formed in long.  The one load is
// unconditional, so a caller that unrolls over its points gets every load issued before the first is waited for.
MOLANN_HD double grid_stencil_term_f64(int p, int d, const double* table, const long (&n)[GRID_MAX_D], const long (&idx)[GRID_MAX_D][4],
                                       const double (&a)[GRID_MAX_D][4], const double (&b)[GRID_MAX_D][4], double (&term)[GRID_MAX_D]) {
#pragma clang fp contract(off)
    long off = 0;
    double wa[GRID_MAX_D], wb[GRID_MAX_D];
#pragma unroll
    for (int k = 0; k < GRID_MAX_D; ++k) {
        wa[k] = 1.0; wb[k] = 0.0;
        if (k < d) {
            const int j = (p >> (2 * k)) & 3;
            off = off * n[k] + grid_pick(idx[k], j);
            wa[k] = grid_pick(a[k], j);
            wb[k] = grid_pick(b[k], j);
        }
    }
    const double T = table[off];
    term[0] = T * (wb[0] * wa[1] * wa[2]);
    term[1] = d > 1 ? T * (wa[0] * wb[1] * wa[2]) : 0.0;
    term[2] = d > 2 ? T * (wa[0] * wa[1] * wb[2]) : 0.0;
    return T * (wa[0] * wa[1] * wa[2]);
}

// A metadynamics deposit onto the table above (metad_deposit_f64_kernel and its host twin): walker a adds the Gaussian hill
// h_a prod_k exp(-1/2 (d_k / sigma_k)^2) to every grid point, d_k = g_k - y_ak with g_k = lower_k + i h_k, wrapped to d - P rint(d / P)
// on a periodic axis (P = n_k h_k; `P` = 0 here: not periodic), where q = sum_k (d_k / sigma_k)^2 <= c2 = cutoff^2 (+inf: everywhere).
// The Gaussian is a product over the axes, so the kernel forms q_k = (d_k / sigma_k)^2 and e_k = exp(-(0.5 q_k)) once per axis index of
// a tile and an entry's term from them: metad_axis_delta_f64, metad_axis_factor_f64, metad_term_f64 (q and the product with k
// ascending).  Nothing is contracted, so the host and the device round alike up to exp.
//
// The table is cut into tiles of metad_tile_extent(d, k) points along axis k, one block each, 256 entries.  metad_axis_reach_f64 is a
// lower bound of q_k over the indices i0..i1 of a tile, from the two ends alone: the computed d is monotone in i but for the one jump a
// wrap can make inside a tile (a tile spans less than a period), so the smallest |d| is an end's, or 0 where the sign changes; division
// and square are monotone too, hence no index of the run has a smaller q_k, in the very numbers the entries use.  A hill whose bounds
// sum (k ascending) to more than c2 adds nothing to the tile: the block skips it, and a tile that every hill skips is not touched.
constexpr int METAD_TILE = 256;
MOLANN_HD constexpr int metad_tile_extent(int d, int k) { return d == 1 ? 256 : d == 2 ? 16 : k == 2 ? 16 : 4; }
MOLANN_HD constexpr int metad_tile_slots(int d) { return d == 1 ? 256 : d == 2 ? 32 : 24; }    // sum_k metad_tile_extent(d, k)
MOLANN_HD constexpr int metad_chunk(int d) { return d == 1 ? 8 : 64; }                            // walkers staged at a time

// h_a = height0 exp(-(V_a inv_dT)), inv_dT = 1 / (kT (biasfactor - 1)); inv_dT = 0: plain metadynamics, h_a = height0
MOLANN_HD double metad_height_f64(double height0, double V, double inv_dT) {
#pragma clang fp contract(off)
    return inv_dT > 0.0 ? height0 * exp(-(V * inv_dT)) : height0;
}
// a walker deposits when V, every y_k and the height are finite and the height > 0 (a NaN fails every comparison)
MOLANN_HD bool metad_walker_valid_f64(double V, const double (&y)[GRID_MAX_D], double h, int d) {
    bool ok = fabs(V) <= 1.7976931348623157e308 && h > 0.0 && h <= 1.7976931348623157e308;
#pragma unroll
    for (int k = 0; k < GRID_MAX_D; ++k)
        if (k < d) ok = ok && fabs(y[k]) <= 1.7976931348623157e308;
    return ok;
}
MOLANN_HD double metad_axis_delta_f64(long i, double y, double lower, double h, double P) {
#pragma clang fp contract(off)
    const double g = lower + (double)i * h;
    double dk = g - y;
    if (P > 0.0) {
        const double turns = rint(dk / P);
        const double whole = P * turns;
        dk = dk - whole;
    }
    return dk;
}
MOLANN_HD double metad_axis_q_f64(double dk, double sigma) {
#pragma clang fp contract(off)
    const double s = dk / sigma;
    return s * s;
}
MOLANN_HD void metad_axis_factor_f64(double dk, double sigma, double& q, double& e) {
#pragma clang fp contract(off)
    q = metad_axis_q_f64(dk, sigma);
    e = exp(-(0.5 * q));
}
MOLANN_HD double metad_axis_reach_f64(long i0, long i1, double y, double lower, double h, double P, double sigma) {
#pragma clang fp contract(off)
    const double lo = metad_axis_delta_f64(i0, y, lower, h, P), hi = metad_axis_delta_f64(i1, y, lower, h, P);
    const double above = lo > 0.0 ? lo : 0.0;      // a run that starts at lo and rises: its smallest |d|, 0 where it crosses 0 ...
    const double below = hi < 0.0 ? -hi : 0.0;     // ... and a run that rises to hi
    double m;
    if (lo <= hi) m = lo > 0.0 ? above : below;    // one run from lo to hi
    else m = above < below ? above : below;        // a wrap inside the tile: lo .. P/2, then -P/2 .. hi (a NaN end: 0, reached)
    return metad_axis_q_f64(m, sigma);
}
// q of an entry or its lower bound over a tile from the axes' q_k, k ascending; the entry's term from the axes' e_k
MOLANN_HD double metad_q_f64(const double (&q)[GRID_MAX_D], int d) {
#pragma clang fp contract(off)
    double s = q[0];
    if (d > 1) s = s + q[1];
    if (d > 2) s = s + q[2];
    return s;
}
MOLANN_HD double metad_term_f64(double h, const double (&e)[GRID_MAX_D], int d) {
#pragma clang fp contract(off)
    double p = e[0];
    if (d > 1) p = p * e[1];
    if (d > 2) p = p * e[2];
    return h * p;
}
// One walker's step of state = (hills, refused, sum_heights, steps, logged, ...), in walker order by one thread: a valid walker is
// counted, its height added and its row (y_k..., sigma_k..., h) appended to log[log_capacity, 2 d + 1] while there is room (a hill past
// the capacity is deposited and counted all the same); any other is refused.  `logged` comes from opes_live_count_f64, so a row index
// lies in [0, log_capacity) whatever the state held.
MOLANN_HD void metad_state_walker_f64(bool valid, double h, const double (&y)[GRID_MAX_D], const double (&sigma)[GRID_MAX_D], int d, double* log,
                                      long log_capacity, double& hills, double& refused, double& sum_heights, long& logged) {
#pragma clang fp contract(off)
    if (!valid) {
        refused = refused + 1.0;
        return;
    }
    hills = hills + 1.0;
    sum_heights = sum_heights + h;
    if (logged < log_capacity) {
        double* row = log + logged * (2 * d + 1);
#pragma unroll
        for (int k = 0; k < GRID_MAX_D; ++k)
            if (k < d) { row[k] = y[k]; row[d + k] = sigma[k]; }
        row[2 * d] = h;
        logged += 1;
    }
}

// Backward of kabsch_rotation: given H, the rotation R it produced and G_R = dL/dR, returns G_H = dL/dH.
// With S = R^T H (symmetric at the optimum) a perturbation dH turns R by dR = R [w]x where
// (tr(S) I - S) w = vee(R^T dH - dH^T R); hence G_H = R [n]x, n = (tr(S) I - S)^-1 vee(M - M^T), M = R^T G_R.
// ([v]x = cross-product matrix of v.)  3x3 products and one 3x3 symmetric solve in T: double, or float where the forward's
// Kabsch is float as well (plans whose items are all invariant under rigid motion).
template <typename T, typename RT = float>
MOLANN_HD void kabsch_rotation_backward_t(const T (&H)[9], const RT (&R)[9], const RT (&GR)[9], RT (&GH)[9]) {
    T S[9], M[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            T s = (T)0, m = (T)0;
#pragma unroll
            for (int k = 0; k < 3; ++k) { s = tfma((T)R[3 * k + a], H[3 * k + b], s); m = tfma((T)R[3 * k + a], (T)GR[3 * k + b], m); }
            S[3 * a + b] = s;
            M[3 * a + b] = m;
        }
    const T s01 = (T)0.5 * (S[1] + S[3]), s02 = (T)0.5 * (S[2] + S[6]), s12 = (T)0.5 * (S[5] + S[7]);
    const T tr = S[0] + S[4] + S[8];
    // B = tr I - S  (symmetric)
    const T b00 = tr - S[0], b11 = tr - S[4], b22 = tr - S[8], b01 = -s01, b02 = -s02, b12 = -s12;
    const T m0 = M[7] - M[5], m1 = M[2] - M[6], m2 = M[3] - M[1]; // vee(M - M^T)
    // n = B^-1 m by the adjugate
    const T c00 = b11 * b22 - b12 * b12, c01 = b02 * b12 - b01 * b22, c02 = b01 * b12 - b02 * b11;
    const T c11 = b00 * b22 - b02 * b02, c12 = b01 * b02 - b00 * b12, c22 = b00 * b11 - b01 * b01;
    const T det = b00 * c00 + b01 * c01 + b02 * c02;
    constexpr T tiny = sizeof(T) == 8 ? (T)1e-300 : (T)1e-30;
    const T inv = (det > tiny || det < -tiny) ? (T)1 / det : (T)0; // ill-defined rotation: no gradient through R
    const T n0 = (c00 * m0 + c01 * m1 + c02 * m2) * inv;
    const T n1 = (c01 * m0 + c11 * m1 + c12 * m2) * inv;
    const T n2 = (c02 * m0 + c12 * m1 + c22 * m2) * inv;
    // G_H = R [n]x ,  [n]x = [[0,-n2,n1],[n2,0,-n0],[-n1,n0,0]]
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const T r0 = R[3 * a], r1 = R[3 * a + 1], r2 = R[3 * a + 2];
        GH[3 * a + 0] = (RT)(r1 * n2 - r2 * n1);
        GH[3 * a + 1] = (RT)(r2 * n0 - r0 * n2);
        GH[3 * a + 2] = (RT)(r0 * n1 - r1 * n0);
    }
}

MOLANN_HD void kabsch_rotation_backward(const double (&H)[9], const float (&R)[9], const float (&GR)[9], float (&GH)[9]) {
    kabsch_rotation_backward_t<double>(H, R, GR, GH);
}

// kabsch_rotation_backward_t in two parts, for a caller with several G_R on one rotation (a Jacobian: one G_R per output).
// _solve_t inverts B = tr(S) I - S once: Binv = the six entries of B's adjugate (00, 01, 02, 11, 12, 22) and 1 / det (0 where the
// rotation is ill-defined).  _apply_t is the part that is linear in G_R: n = adj(B) vee(M - M^T) / det, G_H = R [n]x.  The same
// operations in the same order as kabsch_rotation_backward_t, so solve + apply gives that function's bits.
template <typename T, typename RT = float>
MOLANN_HD void kabsch_rotation_backward_solve_t(const T (&H)[9], const RT (&R)[9], T (&Binv)[7]) {
    T S[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            T s = (T)0;
#pragma unroll
            for (int k = 0; k < 3; ++k) s = tfma((T)R[3 * k + a], H[3 * k + b], s);
            S[3 * a + b] = s;
        }
    const T s01 = (T)0.5 * (S[1] + S[3]), s02 = (T)0.5 * (S[2] + S[6]), s12 = (T)0.5 * (S[5] + S[7]);
    const T tr = S[0] + S[4] + S[8];
    const T b00 = tr - S[0], b11 = tr - S[4], b22 = tr - S[8], b01 = -s01, b02 = -s02, b12 = -s12;
    const T c00 = b11 * b22 - b12 * b12, c01 = b02 * b12 - b01 * b22, c02 = b01 * b12 - b02 * b11;
    const T c11 = b00 * b22 - b02 * b02, c12 = b01 * b02 - b00 * b12, c22 = b00 * b11 - b01 * b01;
    const T det = b00 * c00 + b01 * c01 + b02 * c02;
    constexpr T tiny = sizeof(T) == 8 ? (T)1e-300 : (T)1e-30;
    Binv[0] = c00; Binv[1] = c01; Binv[2] = c02; Binv[3] = c11; Binv[4] = c12; Binv[5] = c22;
    Binv[6] = (det > tiny || det < -tiny) ? (T)1 / det : (T)0;
}
template <typename T, typename RT = float>
MOLANN_HD void kabsch_rotation_backward_apply_t(const RT (&R)[9], const T (&Binv)[7], const RT (&GR)[9], RT (&GH)[9]) {
    T M[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            T m = (T)0;
#pragma unroll
            for (int k = 0; k < 3; ++k) m = tfma((T)R[3 * k + a], (T)GR[3 * k + b], m);
            M[3 * a + b] = m;
        }
    const T m0 = M[7] - M[5], m1 = M[2] - M[6], m2 = M[3] - M[1];
    const T n0 = (Binv[0] * m0 + Binv[1] * m1 + Binv[2] * m2) * Binv[6];
    const T n1 = (Binv[1] * m0 + Binv[3] * m1 + Binv[4] * m2) * Binv[6];
    const T n2 = (Binv[2] * m0 + Binv[4] * m1 + Binv[5] * m2) * Binv[6];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const T r0 = R[3 * a], r1 = R[3 * a + 1], r2 = R[3 * a + 2];
        GH[3 * a + 0] = (RT)(r1 * n2 - r2 * n1);
        GH[3 * a + 1] = (RT)(r2 * n0 - r0 * n2);
        GH[3 * a + 2] = (RT)(r0 * n1 - r1 * n0);
    }
}

// ---- float64 reverse mode of the feature items (the reference differentiates its float64 forward with autograd too) ----
MOLANN_HD V3d operator+(V3d a, V3d b) { return v3d(a.x + b.x, a.y + b.y, a.z + b.z); }
MOLANN_HD V3d operator*(double s, V3d a) { return v3d(s * a.x, s * a.y, s * a.z); }
MOLANN_HD void axpy(V3d& acc, double s, V3d a) { acc.x = fma(s, a.x, acc.x); acc.y = fma(s, a.y, acc.y); acc.z = fma(s, a.z, acc.z); }

// eval_item_backward in double: the same formulas with exact divisions and square roots
MOLANN_HD void eval_item_backward_f64(int type, V3d a0, V3d a1, V3d a2, V3d a3, const double (&g)[3], V3d& ga0, V3d& ga1, V3d& ga2,
                                      V3d& ga3) {
    switch (type) {
    case IT_BOND: {
        const V3d r = a1 - a0;
        const double d2 = dot(r, r);
        const double inv = d2 == 0.0 ? 0.0 : 1.0 / sqrt(d2);   // |r| = 0: subgradient 0; a |r| that is not finite stays so
        axpy(ga1, g[0] * inv, r);
        axpy(ga0, -g[0] * inv, r);
        return;
    }
    case IT_ANGLE_COS:
    case IT_ANGLE_VAL: {
        const V3d u = a0 - a1, v = a2 - a1;
        const double uu = dot(u, u), vv = dot(v, v), uv = dot(u, v);
        if (type == IT_ANGLE_VAL) {   // through w = u x v, as eval_item_backward
            const V3d w = cross(u, v);
            const double gw = g[0] / sqrt(dot(w, w));
            const V3d gu = (gw / uu) * cross(u, w), gv = (gw / vv) * cross(w, v);
            ga0 = ga0 + gu;
            ga2 = ga2 + gv;
            ga1 = ga1 - (gu + gv);
            return;
        }
        const double inv_uv = 1.0 / (sqrt(uu) * sqrt(vv));
        const double c = uv * inv_uv;
        const double gc = g[0];
        V3d gu = v3d(0., 0., 0.), gv = v3d(0., 0., 0.);
        axpy(gu, gc * inv_uv, v); axpy(gu, -gc * c / uu, u);
        axpy(gv, gc * inv_uv, u); axpy(gv, -gc * c / vv, v);
        ga0 = ga0 + gu;
        ga2 = ga2 + gv;
        ga1 = ga1 - (gu + gv);
        return;
    }
    case IT_DIHEDRAL_CS:
    case IT_DIHEDRAL_VAL: {
        const V3d r12 = a1 - a0, r23 = a2 - a1, r34 = a3 - a2;
        const V3d n1 = cross(r12, r23), n2 = cross(r23, r34);
        const double L2 = dot(r23, r23);
        const double L = sqrt(L2);
        const double n1r34 = dot(n1, r34);
        const double C = dot(n1, n2), S = n1r34 * L;
        const double rad2 = fma(C, C, S * S);
        double gC, gS;
        if (type == IT_DIHEDRAL_CS) {
            const double inv_rad = 1.0 / sqrt(rad2);
            const double proj = (g[0] * C + g[1] * S) * inv_rad * inv_rad * inv_rad;
            gC = g[0] * inv_rad - proj * C;
            gS = g[1] * inv_rad - proj * S;
        } else {
            gC = -g[0] * S / rad2;
            gS = g[0] * C / rad2;
        }
        V3d gn1 = gC * n2; axpy(gn1, gS * L, r34);
        const V3d gn2 = gC * n1;
        V3d gr34 = (gS * L) * n1;
        V3d gr23 = (L > 0.0 ? gS * n1r34 / L : 0.0) * r23;
        const V3d gr12 = cross(r23, gn1);
        gr23 = gr23 + cross(gn1, r12) + cross(r34, gn2);
        gr34 = gr34 + cross(gn2, r23);
        ga0 = ga0 - gr12;
        ga1 = ga1 + (gr12 - gr23);
        ga2 = ga2 + (gr23 - gr34);
        ga3 = ga3 + gr34;
        return;
    }
    default: // IT_POSITION
        ga0 = ga0 + v3d(g[0], g[1], g[2]);
        return;
    }
}

// One row of an item's local Jacobian: u[j] = d(output column c of the item) / d(atom j), eval_item_backward_f64 under the unit
// cotangent e_c.  Everything behind the item is linear in the cotangent, so a Jacobian evaluates this once per column of the
// item (at most 3) and combines the rows with d y_k / d feat[col + c] for every output k.
MOLANN_HD void item_unit_backward_f64(int type, V3d a0, V3d a1, V3d a2, V3d a3, int c, V3d (&u)[4]) {
    const double e[3] = {c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = v3d(0., 0., 0.);
    eval_item_backward_f64(type, a0, a1, a2, a3, e, u[0], u[1], u[2], u[3]);
}

// =================================================================================================
// forward mode (tangents: the directional derivatives torch.autograd.forward_ad / torch.func.jvp ask for)
// =================================================================================================
template <typename T> struct VecOf;
template <> struct VecOf<float> { typedef V3 type; };
template <> struct VecOf<double> { typedef V3d type; };
MOLANN_HD float tsqrt(float a) { return sqrtf(a); }
MOLANN_HD double tsqrt(double a) { return sqrt(a); }
MOLANN_HD float tatan2(float y, float x) { return atan2f(y, x); }
MOLANN_HD double tatan2(double y, double x) { return atan2(y, x); }

// One item's values (as eval_item / eval_item_f64) and their derivatives along the atoms' tangents t0..t3.  The forward-mode
// twin of eval_item_backward: exact divisions and square roots, no clamps (the reference's autograd has none either).
template <typename T, typename V = typename VecOf<T>::type>
MOLANN_HD int eval_item_tangent_t(int type, V a0, V a1, V a2, V a3, V t0, V t1, V t2, V t3, T (&out)[3], T (&dout)[3]) {
    switch (type) {
    case IT_BOND: {
        const V r = a1 - a0, dr = t1 - t0;
        const T d = tsqrt(dot(r, r));
        out[0] = d;
        dout[0] = d == (T)0 ? (T)0 : dot(r, dr) / d;  // |r| = 0: the subgradient 0 the backward takes; a |r| that is not finite stays so
        return 1;
    }
    case IT_ANGLE_COS:
    case IT_ANGLE_VAL: {
        const V u = a0 - a1, v = a2 - a1, du = t0 - t1, dv = t2 - t1;
        const T uu = dot(u, u), vv = dot(v, v);
        const T inv_uv = (T)1 / (tsqrt(uu) * tsqrt(vv));
        const T c = dot(u, v) * inv_uv;
        // dc = (du.v + u.dv) / (|u||v|) - c (u.du / |u|^2 + v.dv / |v|^2)
        const T dc = (dot(du, v) + dot(u, dv)) * inv_uv - c * (dot(u, du) / uu + dot(v, dv) / vv);
        if (type == IT_ANGLE_VAL) {   // d theta = (u x w . du / |u|^2 + w x v . dv / |v|^2) / |w|, w = u x v: eval_item_backward's vectors
            const V w = cross(u, v);
            out[0] = tatan2(tsqrt(dot(w, w)), dot(u, v));
            dout[0] = (dot(cross(u, w), du) / uu + dot(cross(w, v), dv) / vv) / tsqrt(dot(w, w));
        } else {
            out[0] = c;
            dout[0] = dc;
        }
        return 1;
    }
    case IT_DIHEDRAL_CS:
    case IT_DIHEDRAL_VAL: {
        const V r12 = a1 - a0, r23 = a2 - a1, r34 = a3 - a2;
        const V d12 = t1 - t0, d23 = t2 - t1, d34 = t3 - t2;
        const V n1 = cross(r12, r23), n2 = cross(r23, r34);
        const V dn1 = cross(d12, r23) + cross(r12, d23), dn2 = cross(d23, r34) + cross(r23, d34);
        const T L = tsqrt(dot(r23, r23));
        const T dL = L > (T)0 ? dot(r23, d23) / L : (T)0;
        const T n1r34 = dot(n1, r34);
        const T C = dot(n1, n2), S = n1r34 * L;
        const T dC = dot(dn1, n2) + dot(n1, dn2);
        const T dS = (dot(dn1, r34) + dot(n1, d34)) * L + n1r34 * dL;
        const T rad2 = C * C + S * S;
        if (type == IT_DIHEDRAL_VAL) { // d atan2(S, C) = (C dS - S dC) / (C^2 + S^2)
            out[0] = tatan2(S, C);
            dout[0] = (C * dS - S * dC) / rad2;
            return 1;
        }
        const T inv_rad = (T)1 / tsqrt(rad2);
        const T proj = (C * dC + S * dS) * inv_rad * inv_rad * inv_rad;   // d(1/rad) = -proj
        out[0] = C * inv_rad;
        out[1] = S * inv_rad;
        dout[0] = dC * inv_rad - C * proj;
        dout[1] = dS * inv_rad - S * proj;
        return 2;
    }
    default: // IT_POSITION
        out[0] = a0.x; out[1] = a0.y; out[2] = a0.z;
        dout[0] = t0.x; dout[1] = t0.y; dout[2] = t0.z;
        return 3;
    }
}

MOLANN_HD int eval_item_tangent(int type, V3 a0, V3 a1, V3 a2, V3 a3, V3 t0, V3 t1, V3 t2, V3 t3, float (&out)[3], float (&dout)[3]) {
    return eval_item_tangent_t<float>(type, a0, a1, a2, a3, t0, t1, t2, t3, out, dout);
}
MOLANN_HD int eval_item_tangent_f64(int type, V3d a0, V3d a1, V3d a2, V3d a3, V3d t0, V3d t1, V3d t2, V3d t3, double (&out)[3],
                                    double (&dout)[3]) {
    return eval_item_tangent_t<double>(type, a0, a1, a2, a3, t0, t1, t2, t3, out, dout);
}

// Tangent of kabsch_rotation: given H, the rotation R it produced and a direction dH, returns dR.  The adjoint of
// kabsch_rotation_backward_t's closed form: with S = R^T H (symmetric at the optimum), dR = R [w]x where
// (tr(S) I - S) w = vee(M - M^T), M = R^T dH.  tr(S) I - S is invertible exactly when the rotation is well defined
// (s2 + d s3 > 0): a planar three-atom alignment needs no special case.  Where it is not, dR = 0, as the backward's G_H.
template <typename T>
MOLANN_HD void kabsch_rotation_tangent_t(const T (&H)[9], const T (&R)[9], const T (&dH)[9], T (&dR)[9]) {
    T S[9], M[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            T s = (T)0, m = (T)0;
#pragma unroll
            for (int k = 0; k < 3; ++k) { s = tfma(R[3 * k + a], H[3 * k + b], s); m = tfma(R[3 * k + a], dH[3 * k + b], m); }
            S[3 * a + b] = s;
            M[3 * a + b] = m;
        }
    const T s01 = (T)0.5 * (S[1] + S[3]), s02 = (T)0.5 * (S[2] + S[6]), s12 = (T)0.5 * (S[5] + S[7]);
    const T tr = S[0] + S[4] + S[8];
    const T b00 = tr - S[0], b11 = tr - S[4], b22 = tr - S[8], b01 = -s01, b02 = -s02, b12 = -s12;
    const T m0 = M[7] - M[5], m1 = M[2] - M[6], m2 = M[3] - M[1];
    const T c00 = b11 * b22 - b12 * b12, c01 = b02 * b12 - b01 * b22, c02 = b01 * b12 - b02 * b11;
    const T c11 = b00 * b22 - b02 * b02, c12 = b01 * b02 - b00 * b12, c22 = b00 * b11 - b01 * b01;
    const T det = b00 * c00 + b01 * c01 + b02 * c02;
    constexpr T tiny = sizeof(T) == 8 ? (T)1e-300 : (T)1e-30;
    const T inv = (det > tiny || det < -tiny) ? (T)1 / det : (T)0;
    const T w0 = (c00 * m0 + c01 * m1 + c02 * m2) * inv;
    const T w1 = (c01 * m0 + c11 * m1 + c12 * m2) * inv;
    const T w2 = (c02 * m0 + c12 * m1 + c22 * m2) * inv;
    // dR = R [w]x ,  [w]x = [[0,-w2,w1],[w2,0,-w0],[-w1,w0,0]]
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const T r0 = R[3 * a], r1 = R[3 * a + 1], r2 = R[3 * a + 2];
        dR[3 * a + 0] = r1 * w2 - r2 * w1;
        dR[3 * a + 1] = r2 * w0 - r0 * w2;
        dR[3 * a + 2] = r0 * w1 - r1 * w0;
    }
}

// =================================================================================================
// second order: tangents of the reverse pass (forward over reverse).  For a cotangent g on the features and a direction u on
// the atoms, d/dx <u, J(x)^T g> = sum_k g_k Hess f_k(x) u is the derivative of the float64 backward along u.  The float64
// backward's closed forms are instantiated on a dual number (value + one tangent): every product, quotient and square root
// carries its first-order term, so the result is the exact derivative of the formulas, with nothing iterative inside
// (the rotation's own tangent dR comes from kabsch_rotation_tangent_t, not from differentiating the solver).
// =================================================================================================
struct Dual {
    double v, d;   // value, tangent
};
MOLANN_HD Dual dual(double v, double d) { Dual r; r.v = v; r.d = d; return r; }
MOLANN_HD Dual operator+(Dual a, Dual b) { return dual(a.v + b.v, a.d + b.d); }
MOLANN_HD Dual operator-(Dual a, Dual b) { return dual(a.v - b.v, a.d - b.d); }
MOLANN_HD Dual operator-(Dual a) { return dual(-a.v, -a.d); }
MOLANN_HD Dual operator-(double s, Dual a) { return dual(s - a.v, -a.d); }
MOLANN_HD Dual operator*(Dual a, Dual b) { return dual(a.v * b.v, fma(a.v, b.d, a.d * b.v)); }
MOLANN_HD Dual operator*(double s, Dual a) { return dual(s * a.v, s * a.d); }
MOLANN_HD Dual operator/(Dual a, Dual b) {
    const double q = a.v / b.v;
    return dual(q, (a.d - q * b.d) / b.v);
}
MOLANN_HD Dual operator/(double s, Dual b) {
    const double q = s / b.v;
    return dual(q, -q * b.d / b.v);
}
MOLANN_HD Dual tfma(Dual a, Dual b, Dual c) { return dual(fma(a.v, b.v, c.v), fma(a.v, b.d, fma(a.d, b.v, c.d))); }
MOLANN_HD Dual tsqrt(Dual a) {
    const double s = sqrt(a.v);
    return dual(s, s > 0.0 ? 0.5 * a.d / s : 0.0);
}
MOLANN_HD double value_of(double a) { return a; }
MOLANN_HD double value_of(Dual a) { return a.v; }

struct V3x {
    Dual x, y, z;
};
MOLANN_HD V3x v3x(Dual x, Dual y, Dual z) { V3x r; r.x = x; r.y = y; r.z = z; return r; }
MOLANN_HD V3x v3x(V3d p, V3d t) { return v3x(dual(p.x, t.x), dual(p.y, t.y), dual(p.z, t.z)); }
MOLANN_HD V3x operator-(V3x a, V3x b) { return v3x(a.x - b.x, a.y - b.y, a.z - b.z); }
MOLANN_HD V3x operator+(V3x a, V3x b) { return v3x(a.x + b.x, a.y + b.y, a.z + b.z); }
MOLANN_HD V3x operator*(Dual s, V3x a) { return v3x(s * a.x, s * a.y, s * a.z); }
MOLANN_HD Dual dot(V3x a, V3x b) { return tfma(a.z, b.z, tfma(a.y, b.y, a.x * b.x)); }
MOLANN_HD V3x cross(V3x a, V3x b) { return v3x(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
MOLANN_HD void axpy(V3x& acc, Dual s, V3x a) { acc.x = tfma(s, a.x, acc.x); acc.y = tfma(s, a.y, acc.y); acc.z = tfma(s, a.z, acc.z); }
MOLANN_HD V3d val3(V3x a) { return v3d(a.x.v, a.y.v, a.z.v); }
MOLANN_HD V3d tan3(V3x a) { return v3d(a.x.d, a.y.d, a.z.d); }

// eval_item_backward_f64's formulas on any scalar T (double, Dual) with vectors V: the same branches, taken on the values
template <typename T, typename V>
MOLANN_HD void eval_item_backward_gen(int type, V a0, V a1, V a2, V a3, const T (&g)[3], V& ga0, V& ga1, V& ga2, V& ga3) {
    const T zero = (T)(0.0 * g[0]);
    switch (type) {
    case IT_BOND: {
        const V r = a1 - a0;
        const T d2 = dot(r, r);
        const T inv = value_of(d2) == 0.0 ? zero : (T)(1.0 / tsqrt(d2));
        axpy(ga1, g[0] * inv, r);
        axpy(ga0, -(g[0] * inv), r);
        return;
    }
    case IT_ANGLE_COS:
    case IT_ANGLE_VAL: {
        const V u = a0 - a1, v = a2 - a1;
        const T uu = dot(u, u), vv = dot(v, v), uv = dot(u, v);
        if (type == IT_ANGLE_VAL) {   // through w = u x v, as eval_item_backward_f64
            const V w = cross(u, v);
            const T gw = g[0] / tsqrt(dot(w, w));
            const V gu = (gw / uu) * cross(u, w), gv = (gw / vv) * cross(w, v);
            ga0 = ga0 + gu;
            ga2 = ga2 + gv;
            ga1 = ga1 - (gu + gv);
            return;
        }
        const T inv_uv = 1.0 / (tsqrt(uu) * tsqrt(vv));
        const T c = uv * inv_uv;
        const T gc = g[0];
        V gu = zero * u, gv = zero * v;
        axpy(gu, gc * inv_uv, v); axpy(gu, -(gc * c / uu), u);
        axpy(gv, gc * inv_uv, u); axpy(gv, -(gc * c / vv), v);
        ga0 = ga0 + gu;
        ga2 = ga2 + gv;
        ga1 = ga1 - (gu + gv);
        return;
    }
    case IT_DIHEDRAL_CS:
    case IT_DIHEDRAL_VAL: {
        const V r12 = a1 - a0, r23 = a2 - a1, r34 = a3 - a2;
        const V n1 = cross(r12, r23), n2 = cross(r23, r34);
        const T L2 = dot(r23, r23);
        const T L = tsqrt(L2);
        const T n1r34 = dot(n1, r34);
        const T C = dot(n1, n2), S = n1r34 * L;
        const T rad2 = tfma(C, C, S * S);
        T gC, gS;
        if (type == IT_DIHEDRAL_CS) {
            const T inv_rad = 1.0 / tsqrt(rad2);
            const T proj = (g[0] * C + g[1] * S) * inv_rad * inv_rad * inv_rad;
            gC = g[0] * inv_rad - proj * C;
            gS = g[1] * inv_rad - proj * S;
        } else {
            gC = -(g[0] * S / rad2);
            gS = g[0] * C / rad2;
        }
        V gn1 = gC * n2; axpy(gn1, gS * L, r34);
        const V gn2 = gC * n1;
        V gr34 = (gS * L) * n1;
        V gr23 = (value_of(L) > 0.0 ? (T)(gS * n1r34 / L) : zero) * r23;
        const V gr12 = cross(r23, gn1);
        gr23 = gr23 + cross(gn1, r12) + cross(r34, gn2);
        gr34 = gr34 + cross(gn2, r23);
        ga0 = ga0 - gr12;
        ga1 = ga1 + (gr12 - gr23);
        ga2 = ga2 + (gr23 - gr34);
        ga3 = ga3 + gr34;
        return;
    }
    default: // IT_POSITION
        ga0.x = ga0.x + g[0]; ga0.y = ga0.y + g[1]; ga0.z = ga0.z + g[2];
        return;
    }
}

// Tangent of eval_item_backward_f64 along the atoms' tangents t0..t3 and a cotangent tangent dg: ga[j] (the gradient itself)
// and dga[j] (its derivative) are ACCUMULATED into.  With dg = 0, dga[j] = sum_k g_k Hess(f_k) t restricted to atom j.
template <typename T = double>
MOLANN_HD void eval_item_backward_tangent_t(int type, V3d a0, V3d a1, V3d a2, V3d a3, V3d t0, V3d t1, V3d t2, V3d t3, const T (&g)[3],
                                            const T (&dg)[3], V3d (&ga)[4], V3d (&dga)[4]) {
    const Dual gd[3] = {dual(g[0], dg[0]), dual(g[1], dg[1]), dual(g[2], dg[2])};
    V3x gx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) gx[j] = v3x(ga[j], dga[j]);
    eval_item_backward_gen<Dual, V3x>(type, v3x(a0, t0), v3x(a1, t1), v3x(a2, t2), v3x(a3, t3), gd, gx[0], gx[1], gx[2], gx[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) { ga[j] = val3(gx[j]); dga[j] = tan3(gx[j]); }
}

// Tangent of kabsch_rotation_backward_t (G_H = R [n]x, n = (tr(S) I - S)^-1 vee(R^T G_R - G_R^T R), S = R^T H) along
// (dH, dR, dG_R): GH receives G_H, dGH its derivative.  dR is the rotation's tangent for dH (kabsch_rotation_tangent_t).
// Where the rotation is ill defined (det of tr(S) I - S below 1e-300) both are zero, as the backward's G_H.
template <typename T = double>
MOLANN_HD void kabsch_rotation_backward_tangent_t(const T (&H)[9], const T (&R)[9], const T (&GR)[9], const T (&dH)[9], const T (&dR)[9],
                                                  const T (&dGR)[9], T (&GH)[9], T (&dGH)[9]) {
    Dual S[9], M[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            Dual s = dual(0., 0.), m = dual(0., 0.);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const Dual r = dual(R[3 * k + a], dR[3 * k + a]);
                s = tfma(r, dual(H[3 * k + b], dH[3 * k + b]), s);
                m = tfma(r, dual(GR[3 * k + b], dGR[3 * k + b]), m);
            }
            S[3 * a + b] = s;
            M[3 * a + b] = m;
        }
    const Dual s01 = 0.5 * (S[1] + S[3]), s02 = 0.5 * (S[2] + S[6]), s12 = 0.5 * (S[5] + S[7]);
    const Dual tr = S[0] + S[4] + S[8];
    const Dual b00 = tr - S[0], b11 = tr - S[4], b22 = tr - S[8], b01 = -s01, b02 = -s02, b12 = -s12;
    const Dual m0 = M[7] - M[5], m1 = M[2] - M[6], m2 = M[3] - M[1];
    const Dual c00 = b11 * b22 - b12 * b12, c01 = b02 * b12 - b01 * b22, c02 = b01 * b12 - b02 * b11;
    const Dual c11 = b00 * b22 - b02 * b02, c12 = b01 * b02 - b00 * b12, c22 = b00 * b11 - b01 * b01;
    const Dual det = b00 * c00 + b01 * c01 + b02 * c02;
    const bool ok = det.v > 1e-300 || det.v < -1e-300;
    const Dual inv = ok ? 1.0 / det : dual(0., 0.);
    const Dual n0 = (c00 * m0 + c01 * m1 + c02 * m2) * inv;
    const Dual n1 = (c01 * m0 + c11 * m1 + c12 * m2) * inv;
    const Dual n2 = (c02 * m0 + c12 * m1 + c22 * m2) * inv;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const Dual r0 = dual(R[3 * a], dR[3 * a]), r1 = dual(R[3 * a + 1], dR[3 * a + 1]), r2 = dual(R[3 * a + 2], dR[3 * a + 2]);
        const Dual g0 = r1 * n2 - r2 * n1, g1 = r2 * n0 - r0 * n2, g2 = r0 * n1 - r1 * n0;
        GH[3 * a] = g0.v; GH[3 * a + 1] = g1.v; GH[3 * a + 2] = g2.v;
        dGH[3 * a] = g0.d; dGH[3 * a + 1] = g1.d; dGH[3 * a + 2] = g2.d;
    }
}

} // namespace molann
