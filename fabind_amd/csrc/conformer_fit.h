// The rigid fit of csrc/conformer_fit.hip, shared with csrc/pose_relax.hip: the fixed-order wave sum, the packed-triangle index and
// Horn's quaternion method (fit_horn), every lane ending with the same bits.
#pragma once
#include "common.h"

#define FIT_SWEEPS 16

__device__ __forceinline__ double fit_wave_sum(double v) {             // all 64 lanes get the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int fit_tri(int i, int j) { return i * (i + 1) / 2 + j; }      // j <= i

struct FitRigid { double R[3][3], cp[3], cy[3], q[4]; };               // image = R (p - cp) + cy; R = R(q), q the unit quaternion

// Horn 1987: P(i, d) / Y(i, d) = coordinate d of atom i as double.  Every lane ends with the same bits.
template <typename PF, typename YF>
__device__ __forceinline__ void fit_horn(int n, int ln, PF P, YF Y, FitRigid& r) {
    double c[6] = {0., 0., 0., 0., 0., 0.};
    for (int i = ln; i < n; i += 64) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { c[d] += P(i, d); c[3 + d] += Y(i, d); }
    }
#pragma unroll
    for (int d = 0; d < 6; ++d) c[d] = fit_wave_sum(c[d]) / (double)n;
    double S[3][3] = {{0., 0., 0.}, {0., 0., 0.}, {0., 0., 0.}};
    for (int i = ln; i < n; i += 64) {
        const double p[3] = {P(i, 0) - c[0], P(i, 1) - c[1], P(i, 2) - c[2]};
        const double y[3] = {Y(i, 0) - c[3], Y(i, 1) - c[4], Y(i, 2) - c[5]};
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int z = 0; z < 3; ++z) S[x][z] += p[x] * y[z];
    }
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int z = 0; z < 3; ++z) S[x][z] = fit_wave_sum(S[x][z]);
    double a[4][4], v[4][4];
    a[0][0] = S[0][0] + S[1][1] + S[2][2];
    a[1][1] = S[0][0] - S[1][1] - S[2][2];
    a[2][2] = -S[0][0] + S[1][1] - S[2][2];
    a[3][3] = -S[0][0] - S[1][1] + S[2][2];
    a[0][1] = a[1][0] = S[1][2] - S[2][1];
    a[0][2] = a[2][0] = S[2][0] - S[0][2];
    a[0][3] = a[3][0] = S[0][1] - S[1][0];
    a[1][2] = a[2][1] = S[0][1] + S[1][0];
    a[1][3] = a[3][1] = S[2][0] + S[0][2];
    a[2][3] = a[3][2] = S[1][2] + S[2][1];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int z = 0; z < 4; ++z) v[x][z] = x == z ? 1. : 0.;
    for (int sweep = 0; sweep < FIT_SWEEPS; ++sweep) {                 // wave-uniform throughout
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[0][3]) + fabs(a[1][2]) + fabs(a[1][3]) + fabs(a[2][3]);
        if (off == 0.) break;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = a[p][q];
                if (apq == 0.) continue;
                const double g = 100. * fabs(apq);
                if (fabs(a[p][p]) + g == fabs(a[p][p]) && fabs(a[q][q]) + g == fabs(a[q][q])) {
                    a[p][q] = a[q][p] = 0.;
                    continue;
                }
                const double theta = (a[q][q] - a[p][p]) / (2. * apq);
                const double t = (theta >= 0. ? 1. : -1.) / (fabs(theta) + sqrt(theta * theta + 1.));
                const double cs = 1. / sqrt(t * t + 1.), sn = t * cs;
#pragma unroll
                for (int x = 0; x < 4; ++x) {                          // a <- a G, v <- v G
                    const double xp = a[x][p], xq = a[x][q];
                    a[x][p] = cs * xp - sn * xq;
                    a[x][q] = sn * xp + cs * xq;
                    const double vp = v[x][p], vq = v[x][q];
                    v[x][p] = cs * vp - sn * vq;
                    v[x][q] = sn * vp + cs * vq;
                }
#pragma unroll
                for (int x = 0; x < 4; ++x) {                          // a <- G^T a
                    const double px = a[p][x], qx = a[q][x];
                    a[p][x] = cs * px - sn * qx;
                    a[q][x] = sn * px + cs * qx;
                }
                a[p][q] = a[q][p] = 0.;
            }
    }
    double best = a[0][0], q[4] = {v[0][0], v[1][0], v[2][0], v[3][0]};
#pragma unroll
    for (int x = 1; x < 4; ++x)
        if (a[x][x] > best) {                                          // the first of equal eigenvalues
            best = a[x][x];
#pragma unroll
            for (int z = 0; z < 4; ++z) q[z] = v[z][x];
        }
    const double qn = 1. / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double q0 = q[0] * qn, qx = q[1] * qn, qy = q[2] * qn, qz = q[3] * qn;
    r.R[0][0] = q0 * q0 + qx * qx - qy * qy - qz * qz; r.R[0][1] = 2. * (qx * qy - q0 * qz); r.R[0][2] = 2. * (qx * qz + q0 * qy);
    r.R[1][0] = 2. * (qy * qx + q0 * qz); r.R[1][1] = q0 * q0 - qx * qx + qy * qy - qz * qz; r.R[1][2] = 2. * (qy * qz - q0 * qx);
    r.R[2][0] = 2. * (qz * qx - q0 * qy); r.R[2][1] = 2. * (qz * qy + q0 * qx); r.R[2][2] = q0 * q0 - qx * qx - qy * qy + qz * qz;
#pragma unroll
    for (int d = 0; d < 3; ++d) { r.cp[d] = c[d]; r.cy[d] = c[3 + d]; }
    r.q[0] = q0; r.q[1] = qx; r.q[2] = qy; r.q[3] = qz;
}

__device__ __forceinline__ double fit_image(const FitRigid& r, double px, double py, double pz, int d) {
    return (r.R[d][0] * (px - r.cp[0]) + r.R[d][1] * (py - r.cp[1]) + r.R[d][2] * (pz - r.cp[2])) + r.cy[d];
}

// sp <- the centred start conformer sx0 with the torsions applied one after another as relative rotations by ang[t] in float32: the
// rule and the arithmetic of conformer_perturb_kernel.  One wave; the pose is complete and visible to every lane on return.
__device__ __forceinline__ void fit_torsions(int n, int T, int ln, const float* sx0, const int* squad, const uint32_t* smask,
                                             const float* ang, float* sp) {
    for (int i = ln; i < 3 * n; i += 64) sp[i] = sx0[i];
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const int qj = squad[4 * t + 1], qk = squad[4 * t + 2];
        if (qj < 0) continue;                                          // wave-uniform: an atom id out of range (marked on load)
        const float pjx = sp[3 * qj], pjy = sp[3 * qj + 1], pjz = sp[3 * qj + 2];
        const float b2x = sp[3 * qk] - pjx, b2y = sp[3 * qk + 1] - pjy, b2z = sp[3 * qk + 2] - pjz;
        __syncthreads();                                               // every lane holds the axis before any atom moves
        const float l2 = b2x * b2x + b2y * b2y + b2z * b2z;
        if (l2 == 0.f) continue;                                       // wave-uniform
        float sn, cs;
        sincosf(ang[t], &sn, &cs);
        const float inv = 1.0f / sqrtf(l2);
        const float ux = b2x * inv, uy = b2y * inv, uz = b2z * inv;
        const uint32_t* sd = smask + 8 * t;                            // side without k
        for (int a = ln; a < n; a += 64) {
            if ((sd[a >> 5] >> (a & 31)) & 1u) {
                const float vx = sp[3 * a] - pjx, vy = sp[3 * a + 1] - pjy, vz = sp[3 * a + 2] - pjz;
                const float d = (ux * vx + uy * vy + uz * vz) * (1.0f - cs);
                const float wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
                sp[3 * a] = pjx + (vx * cs + wx * sn + ux * d);
                sp[3 * a + 1] = pjy + (vy * cs + wy * sn + uy * d);
                sp[3 * a + 2] = pjz + (vz * cs + wz * sn + uz * d);
            }
        }
        __syncthreads();
    }
}
