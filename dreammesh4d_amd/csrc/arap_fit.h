// arap_fit.h -- the rotation that best fits a one-ring covariance: R = argmax over SO(3) of tr(R S).
//
// The reference (custom/threestudio-dreammesh4d/utils/arap_utils.py:204-214) takes S = U diag(sig) W^T by a batched SVD, sets
// R = W U^T and, where det(R) <= 0, flips the column of U that belongs to the smallest singular value.  Both branches give the
// same thing: R = w1 u1^T + w2 u2^T + d (w1 x w2)(u1 x u2)^T with d = +-1, the proper rotation that maximises tr(R S) (Kabsch /
// Horn).  On a mesh the one-rings are nearly planar (sig3 / sig1 ~ 1e-3 ... 1e-2), so the flip is taken at every other vertex and
// u3, w3 are the worst-conditioned part of the SVD; R itself is conditioned by gap = (sig2 + d sig3) / sig1 alone.
//
// So no SVD here: Horn's closed form (J. Opt. Soc. Am. A 4(4), 1987, section 4) turns the maximisation into the dominant eigenvector
// of a symmetric 4 x 4 matrix N(S) -- tr(R(q) S) = q^T N q for the unit quaternion q = (q0, qx, qy, qz) -- whose two largest
// eigenvalues are sig1 + sig2 + d sig3 and sig1 - sig2 - d sig3: their distance is exactly 2 gap sig1, and the determinant sign
// never has to be decided.  The eigenvector comes from cyclic Jacobi rotations (each one exactly orthogonal up to rounding, no
// squaring of S), in double: MI355X runs double FMAs at half the float rate, the fit is off the training step's path, and R comes
// out as the double fit rounded once to float32 -- nothing to argue about float32 eigenvectors at gap ~ 1e-4.
#pragma once

#if defined(__HIPCC__)
#define DM4D_HD __host__ __device__ __forceinline__
#else
#define DM4D_HD inline
#endif

namespace dm4d {

constexpr int kJacobiSweeps = 6;      // cyclic Jacobi converges quadratically: on 80 k matrices (Gaussian, near-planar with
                                      // sig3 / sig1 < 1e-3, gap < 1e-4, scaled by 1e+-20) R moves by 1e-4 from sweep 4 to 5, by
                                      // 7e-14 from 5 to 6 and not at all from 6 on -- a sweep more than the float32 output
                                      // needs (a sweep is ~3 us of k_arap_fit's 68 at 16.7k vertices x 14); a fixed count keeps a wave together

// S row-major, S[3 r + c] = sum_j w_ij e_ij[r] e'_ij[c] (rest edge x deformed edge).  Writes the row-major rotation with
// e' ~ R e.  S = 0 gives the identity (all eigenvalues tie, the first is taken: q = (1, 0, 0, 0)), as torch.svd of zeros does.
DM4D_HD void fit_rotation(const double S[9], double R[9])
{
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double A[4][4] = {{(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {0.0, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz},
                      {0.0, 0.0, (Syy - Sxx) - Szz, Syz + Szy},
                      {0.0, 0.0, 0.0, (Szz - Sxx) - Syy}};      // upper triangle only: A[p][q] with p <= q
    double Q[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[p][q];
                if (apq != 0.0) {
                    // tan of the rotation angle: the smaller root of t^2 + 2 theta t - 1 = 0 (a huge theta gives t = 0)
                    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                    A[p][p] -= t * apq;
                    A[q][q] += t * apq;
                    A[p][q] = 0.0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (k != p && k != q) {
                            double &akp = k < p ? A[k][p] : A[p][k], &akq = k < q ? A[k][q] : A[q][k];
                            const double x = akp, y = akq;
                            akp = c * x - s * y;
                            akq = s * x + c * y;
                        }
                        const double x = Q[k][p], y = Q[k][q];
                        Q[k][p] = c * x - s * y;
                        Q[k][q] = s * x + c * y;
                    }
                }
            }
        }
    }
    double best = A[0][0], q0 = Q[0][0], qx = Q[1][0], qy = Q[2][0], qz = Q[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (A[k][k] > best) { best = A[k][k]; q0 = Q[0][k]; qx = Q[1][k]; qy = Q[2][k]; qz = Q[3][k]; }
    const double n = 1.0 / sqrt(((q0 * q0 + qx * qx) + qy * qy) + qz * qz);
    q0 *= n; qx *= n; qy *= n; qz *= n;
    R[0] = ((q0 * q0 + qx * qx) - qy * qy) - qz * qz; R[1] = 2.0 * (qx * qy - q0 * qz); R[2] = 2.0 * (qx * qz + q0 * qy);
    R[3] = 2.0 * (qy * qx + q0 * qz); R[4] = ((q0 * q0 - qx * qx) + qy * qy) - qz * qz; R[5] = 2.0 * (qy * qz - q0 * qx);
    R[6] = 2.0 * (qz * qx - q0 * qy); R[7] = 2.0 * (qz * qy + q0 * qx); R[8] = ((q0 * q0 - qx * qx) - qy * qy) + qz * qz;
}

DM4D_HD double det3(const double S[9])
{
    return (S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6])) + S[2] * (S[3] * S[7] - S[4] * S[6]);
}

}  // namespace dm4d
