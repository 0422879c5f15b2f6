// sh.h -- real spherical harmonics of degree 0..3 in a unit direction (x, y, z): the 16 basis functions in the
// sign and normalisation convention of the published 3D Gaussian Splatting colour model (what the reference's eval_sh
// computes, C/geometry/sugar.py:733-820), and their partial derivatives with respect to x, y and z taken as free
// variables (the normalisation of the direction is the caller's chain).
//
//   l = 0   B0  =  k0
//   l = 1   B1  = -k1 y                 B2  =  k1 z                      B3  = -k1 x
//   l = 2   B4  =  k2a xy               B5  = -k2a yz                    B6  =  k2b (2zz - xx - yy)
//           B7  = -k2a xz               B8  =  k2c (xx - yy)
//   l = 3   B9  = -k3a y (3xx - yy)     B10 =  k3b xyz                   B11 = -k3c y (4zz - xx - yy)
//           B12 =  k3d z (2zz - 3xx - 3yy)                               B13 = -k3c x (4zz - xx - yy)
//           B14 =  k3e z (xx - yy)      B15 = -k3a x (xx - 3yy)
//
//   k0 = 1/2 sqrt(1/pi), k1 = sqrt(3/(4 pi)), k2a = 1/2 sqrt(15/pi), k2b = 1/4 sqrt(5/pi), k2c = 1/4 sqrt(15/pi),
//   k3a = 1/4 sqrt(35/(2 pi)), k3b = 1/2 sqrt(105/pi), k3c = 1/4 sqrt(21/(2 pi)), k3d = 1/4 sqrt(7/pi), k3e = 1/4 sqrt(105/pi)
//
// Plain float32, one rounding per written operation (-ffp-contract=off like the rest of csrc/).
#pragma once
#include "common.h"

namespace dm4d {

constexpr float kSh0 = 0.28209479177387814f;
constexpr float kSh1 = 0.4886025119029199f;
constexpr float kSh2a = 1.0925484305920792f;
constexpr float kSh2b = 0.31539156525252005f;
constexpr float kSh2c = 0.5462742152960396f;
constexpr float kSh3a = 0.5900435899266435f;
constexpr float kSh3b = 2.890611442640554f;
constexpr float kSh3c = 0.4570457994644658f;
constexpr float kSh3d = 0.3731763325901154f;
constexpr float kSh3e = 1.445305721320277f;

constexpr int kShMaxDegree = 3;
constexpr int sh_count(int degree) { return (degree + 1) * (degree + 1); }

template <int DEG>
__device__ __forceinline__ void sh_basis(const float x, const float y, const float z, float (&B)[sh_count(DEG)])
{
    B[0] = kSh0;
    if constexpr (DEG >= 1) {
        B[1] = -kSh1 * y;
        B[2] = kSh1 * z;
        B[3] = -kSh1 * x;
    }
    if constexpr (DEG >= 2) {
        const float xx = x * x, yy = y * y, zz = z * z;
        B[4] = kSh2a * (x * y);
        B[5] = -kSh2a * (y * z);
        B[6] = kSh2b * ((2.f * zz - xx) - yy);
        B[7] = -kSh2a * (x * z);
        B[8] = kSh2c * (xx - yy);
        if constexpr (DEG >= 3) {
            const float q = (4.f * zz - xx) - yy;
            B[9] = (-kSh3a * y) * (3.f * xx - yy);
            B[10] = (kSh3b * (x * y)) * z;
            B[11] = (-kSh3c * y) * q;
            B[12] = (kSh3d * z) * ((2.f * zz - 3.f * xx) - 3.f * yy);
            B[13] = (-kSh3c * x) * q;
            B[14] = (kSh3e * z) * (xx - yy);
            B[15] = (-kSh3a * x) * (xx - 3.f * yy);
        }
    }
}

// dB_k/dx, dB_k/dy, dB_k/dz of the polynomials above
template <int DEG>
__device__ __forceinline__ void sh_basis_grad(const float x, const float y, const float z, float (&dx)[sh_count(DEG)],
                                              float (&dy)[sh_count(DEG)], float (&dz)[sh_count(DEG)])
{
    dx[0] = 0.f; dy[0] = 0.f; dz[0] = 0.f;
    if constexpr (DEG >= 1) {
        dx[1] = 0.f;    dy[1] = -kSh1; dz[1] = 0.f;
        dx[2] = 0.f;    dy[2] = 0.f;   dz[2] = kSh1;
        dx[3] = -kSh1;  dy[3] = 0.f;   dz[3] = 0.f;
    }
    if constexpr (DEG >= 2) {
        dx[4] = kSh2a * y;          dy[4] = kSh2a * x;          dz[4] = 0.f;
        dx[5] = 0.f;                dy[5] = -kSh2a * z;         dz[5] = -kSh2a * y;
        dx[6] = (-2.f * kSh2b) * x; dy[6] = (-2.f * kSh2b) * y; dz[6] = (4.f * kSh2b) * z;
        dx[7] = -kSh2a * z;         dy[7] = 0.f;                dz[7] = -kSh2a * x;
        dx[8] = (2.f * kSh2c) * x;  dy[8] = (-2.f * kSh2c) * y; dz[8] = 0.f;
    }
    if constexpr (DEG >= 3) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        dx[9] = (-6.f * kSh3a) * xy;
        dy[9] = (-3.f * kSh3a) * (xx - yy);
        dz[9] = 0.f;
        dx[10] = kSh3b * yz;
        dy[10] = kSh3b * xz;
        dz[10] = kSh3b * xy;
        dx[11] = (2.f * kSh3c) * xy;
        dy[11] = -kSh3c * ((4.f * zz - xx) - 3.f * yy);
        dz[11] = (-8.f * kSh3c) * yz;
        dx[12] = (-6.f * kSh3d) * xz;
        dy[12] = (-6.f * kSh3d) * yz;
        dz[12] = (3.f * kSh3d) * ((2.f * zz - xx) - yy);
        dx[13] = -kSh3c * ((4.f * zz - 3.f * xx) - yy);
        dy[13] = (2.f * kSh3c) * xy;
        dz[13] = (-8.f * kSh3c) * xz;
        dx[14] = (2.f * kSh3e) * xz;
        dy[14] = (-2.f * kSh3e) * yz;
        dz[14] = kSh3e * (xx - yy);
        dx[15] = (-3.f * kSh3a) * (xx - yy);
        dy[15] = (6.f * kSh3a) * xy;
        dz[15] = 0.f;
    }
}

// unit direction from `campos` to `p`; a zero vector (and len = 0) when they coincide
__device__ __forceinline__ void sh_direction(const float px, const float py, const float pz, const float cx, const float cy,
                                             const float cz, float &x, float &y, float &z, float &len)
{
    const float ux = px - cx, uy = py - cy, uz = pz - cz;
    len = sqrtf((ux * ux + uy * uy) + uz * uz);
    const bool ok = len > 0.f;
    x = ok ? ux / len : 0.f;
    y = ok ? uy / len : 0.f;
    z = ok ? uz / len : 0.f;
}

}  // namespace dm4d
