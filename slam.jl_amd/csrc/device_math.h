// device_math.h -- scalar geometry of the range-bearing observation model.
// Always evaluated in double, whatever the storage type of x and P.
#pragma once
#include <hip/hip_runtime.h>

#include "wave_reduce.h"

#define SLAM_PI_D 3.14159265358979323846

// mpi_to_pi, src/common.jl:102-110: ONE conditional wrap, not a modulo.
__host__ __device__ inline double mpi_to_pi_d(double phi) {
    if (phi > SLAM_PI_D) return phi - 2.0 * SLAM_PI_D;
    if (phi < -SLAM_PI_D) return phi + 2.0 * SLAM_PI_D;
    return phi;
}

// The non-zero part of predict_observation (src/common.jl:146-162) for the
// landmark at (lx, ly) seen from pose (xv, yv, phi).
//   zp = [d; atan2(dy,dx) - phi]        (bearing NOT wrapped, :152)
//   Hv = [-dx/d -dy/d 0; dy/d2 -dx/d2 -1]   (row-major here: Hv[row*3+col])
//   Hf = [ dx/d  dy/d;  -dy/d2  dx/d2]      (row-major: Hf[row*2+col])
struct ObsModel {
    double zp[2];
    double Hv[6];
    double Hf[4];
};

__host__ __device__ inline ObsModel obs_model(double xv, double yv, double phi, double lx, double ly) {
    ObsModel o;
    const double dx = lx - xv;
    const double dy = ly - yv;
    const double d2 = dx * dx + dy * dy;
    const double d = sqrt(d2);
    o.zp[0] = d;
    o.zp[1] = atan2(dy, dx) - phi;
    const double xd = dx / d, yd = dy / d, xd2 = dx / d2, yd2 = dy / d2;
    o.Hv[0] = -xd;  o.Hv[1] = -yd;  o.Hv[2] = 0.0;
    o.Hv[3] = yd2;  o.Hv[4] = -xd2; o.Hv[5] = -1.0;
    o.Hf[0] = xd;   o.Hf[1] = yd;
    o.Hf[2] = -yd2; o.Hf[3] = xd2;
    return o;
}

// ---- the pair arithmetic of the gating sweep (ekf_gate.hip) and of joint compatibility (ekf_jc.hip) ----------------------------
struct PairConst {        // per-landmark, observation-independent
    double zp0, zp1;
    double s00, s01, s10, s11;
    double det, logdet;
    double qa, qb, qc;    // nis = qa*v0^2 + qb*v0*v1 + qc*v1^2  (inv(S) folded in once per landmark)
};

// S = Hv Pvv Hv' + Hv Pvf Hf' + Hf Pfv Hv' + Hf Pff Hf' + R  (2x2), from the
// 5x5 sub-block of P.  pvv is row-major 3x3; pfv[a][c] = P[f+a][c]; pff row-major.
__device__ inline PairConst pair_const(const ObsModel& om, const double* pvv, const double pfv[2][3],
                                       const double pff[4], const double R[4]) {
    PairConst pc;
    pc.zp0 = om.zp[0];
    pc.zp1 = om.zp[1];
    double A[2][3];   // Hv * Pvv
    double B[2][2];   // Hv * Pvf,  Pvf[c][a] = pfv[a][c]
    double Cc[2][3];  // Hf * Pfv
    double D[2][2];   // Hf * Pff
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            A[r][c] = om.Hv[r * 3 + 0] * pvv[0 * 3 + c] + om.Hv[r * 3 + 1] * pvv[1 * 3 + c] +
                      om.Hv[r * 3 + 2] * pvv[2 * 3 + c];
            Cc[r][c] = om.Hf[r * 2 + 0] * pfv[0][c] + om.Hf[r * 2 + 1] * pfv[1][c];
        }
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            B[r][a] = om.Hv[r * 3 + 0] * pfv[a][0] + om.Hv[r * 3 + 1] * pfv[a][1] + om.Hv[r * 3 + 2] * pfv[a][2];
            D[r][a] = om.Hf[r * 2 + 0] * pff[0 * 2 + a] + om.Hf[r * 2 + 1] * pff[1 * 2 + a];
        }
    }
    double S[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            double s = A[r][0] * om.Hv[q * 3 + 0] + A[r][1] * om.Hv[q * 3 + 1] + A[r][2] * om.Hv[q * 3 + 2];
            s += B[r][0] * om.Hf[q * 2 + 0] + B[r][1] * om.Hf[q * 2 + 1];
            s += Cc[r][0] * om.Hv[q * 3 + 0] + Cc[r][1] * om.Hv[q * 3 + 1] + Cc[r][2] * om.Hv[q * 3 + 2];
            s += D[r][0] * om.Hf[q * 2 + 0] + D[r][1] * om.Hf[q * 2 + 1];
            S[r][q] = s + R[q * 2 + r];       // R column-major: R[r][q] = R[q*2+r]
        }
    pc.s00 = S[0][0]; pc.s01 = S[0][1]; pc.s10 = S[1][0]; pc.s11 = S[1][1];
    pc.det = pc.s00 * pc.s11 - pc.s01 * pc.s10;
    pc.logdet = log(pc.det);
    const double rdet = 1.0 / pc.det;
    pc.qa = pc.s11 * rdet;
    pc.qb = -(pc.s01 + pc.s10) * rdet;
    pc.qc = pc.s00 * rdet;
    return pc;
}

// nis = v' inv(S) v  (src/data-association.jl:60), nd = nis + log det S (:61)
__device__ inline void pair_eval(const PairConst& pc, double z0, double z1, double& nis, double& nd) {
    const double v0 = z0 - pc.zp0;
    const double v1 = mpi_to_pi_d(z1 - pc.zp1);        // :57
    nis = pc.qa * v0 * v0 + pc.qb * v0 * v1 + pc.qc * v1 * v1;
    nd = nis + pc.logdet;
}

// ---- storage of the covariance: TILE-MAJOR, block lower -----------------------------------------------------------------
// Only the square tiles (edge E = 2^L: 128 for fp32, 64 for fp64) ON and BELOW the diagonal exist (the rank-k down-date
// updates one triangle, like BLAS syrk).  Each tile is one contiguous E x E column-major block; the tiles of column band J
// follow each other, I = J (the diagonal tile, stored complete and symmetric), J + 1, ..., T - 1, band after band:
//     tile (I, J) is block number  J*T - J*(J-1)/2 + (I - J),      T = ld >> L  tile rows of the ALLOCATION.
// The down-date walks the bands in this order, so its P traffic is ONE linear stream through memory -- a 128 x 128 tile of a
// column-major matrix is 128 runs of 512 bytes 80 KB apart, which the memory system serves 7-10 % slower
// (tools/micro_tilewalk.hip) -- and half of the square matrix is never allocated.  `ld` (= npad, a multiple of 128) only
// carries T; every access to P goes through p_off / sym_at / p_store_sym.
template <typename T>
constexpr int kTileLog2 = sizeof(T) == 4 ? 7 : 6;      // L of a state whose elements are T

__host__ __device__ inline size_t tile_base(int I, int J, int T, int L) {
    return ((size_t)J * (size_t)T - (size_t)J * (size_t)(J - 1) / 2 + (size_t)(I - J)) << (2 * L);
}

// tile_base's inverse: tile q of the Tw (Tw + 1) / 2 tiles of the leading Tw tile rows, numbered band after band:
// base(J) = J Tw - J (J - 1) / 2
__device__ __forceinline__ void tile_of(long long q, int Tw, int* I, int* J) {
    const double b = 2.0 * Tw + 1.0;
    int j = (int)((b - sqrt(b * b - 8.0 * (double)q)) * 0.5);
    if (j < 0) j = 0;
    if (j > Tw - 1) j = Tw - 1;
    while (j > 0 && (long long)j * Tw - (long long)j * (j - 1) / 2 > q) --j;
    while (j < Tw - 1 && (long long)(j + 1) * Tw - (long long)(j + 1) * j / 2 <= q) ++j;
    *J = j;
    *I = j + (int)(q - ((long long)j * Tw - (long long)j * (j - 1) / 2));
}

// offset of element (r, c); requires (r >> L) >= (c >> L)
__host__ __device__ inline size_t p_off(int ld, int L, int r, int c) {
    const int m = (1 << L) - 1;
    return tile_base(r >> L, c >> L, ld >> L, L) + ((size_t)(c & m) << L) + (size_t)(r & m);
}

// element (r, c) of the symmetric matrix, from whichever of (r, c) / (c, r) lies in a stored tile
template <typename T>
__device__ inline T sym_at(const T* __restrict__ P, int ld, int tile_log2, int r, int c) {
    return ((r >> tile_log2) >= (c >> tile_log2)) ? P[p_off(ld, tile_log2, r, c)] : P[p_off(ld, tile_log2, c, r)];
}

// store P[r, c] = P[c, r] = v wherever those positions exist (both inside a diagonal tile, one otherwise)
template <typename T>
__device__ inline void p_store_sym(T* __restrict__ P, int ld, int tile_log2, int r, int c, T v) {
    if ((r >> tile_log2) >= (c >> tile_log2)) P[p_off(ld, tile_log2, r, c)] = v;
    if ((c >> tile_log2) >= (r >> tile_log2) && r != c) P[p_off(ld, tile_log2, c, r)] = v;
}

// store P[r, c] = v if that position exists (its mirror is the caller's business)
template <typename T>
__device__ inline void p_store(T* __restrict__ P, int ld, int tile_log2, int r, int c, T v) {
    if ((r >> tile_log2) >= (c >> tile_log2)) P[p_off(ld, tile_log2, r, c)] = v;
}

// ---- the landmarks' 2 x 2 diagonal blocks, packed (SURVEY 7 "hard parts") -------------------------------------------------
// side[0][j] = P[f, f], side[1][j] = P[f+1, f], side[2][j] = P[f+1, f+1] with f = 3 + 2 j, three rows of side_n values each
// in the state's dtype.  In the tile-major matrix these entries sit on the diagonals of the diagonal tiles, 129 elements
// apart: every landmark of the gating sweep touched two 128-byte lines of its own for 12 useful bytes (6.5x the sweep's
// algorithmic bytes).  The side array is kept by EVERY writer of those entries -- the state upload (pack_kernel),
// add_features (augment_kernel) and the diagonal-tile epilogues of the down-dates -- through side_note(), and read by the
// sweep (ekf_gate.hip) as three coalesced rows.  The matrix itself stays complete: every other reader uses P.
template <typename T>
__device__ __forceinline__ void side_note(T* __restrict__ side, int side_n, int r, int c, T v) {
    if (c < 3) return;
    const int o = c - 3, j = o >> 1;
    if (r == c) side[(size_t)((o & 1) ? 2 : 0) * side_n + j] = v;
    else if (r == c + 1 && !(o & 1)) side[(size_t)side_n + j] = v;
}

// ---- groups of state indices: g = 0 the pose pair (0, 1), g = 1 the heading (2), g >= 2 the landmark pair (2g - 1, 2g) -------------
__host__ __device__ inline int grp_first(int g) { return g < 2 ? 2 * g : 2 * g - 1; }
__host__ __device__ inline int grp_size(int g) { return g == 1 ? 1 : 2; }

// ---- a tile of P on the matrix cores: one MFMA block is MB x MB over KS values of k, NREG accumulator registers per lane; lane
// (li = lane & (MB - 1), half = lane >> LSH) holds the B dimension li and, in register reg, the A dimension out_i(reg, half) ------
template <typename T> struct MfmaTile;
template <> struct MfmaTile<float> {
    static constexpr int L = kTileLog2<float>, MB = 32, KS = 2, NREG = 16, LSH = 5;
    typedef float Acc __attribute__((ext_vector_type(16)));
    static __device__ __forceinline__ Acc mfma(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int out_i(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }     // index of the A dimension
};
template <> struct MfmaTile<double> {
    static constexpr int L = kTileLog2<double>, MB = 16, KS = 4, NREG = 4, LSH = 4;
    typedef double Acc __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ Acc mfma(double a, double b, Acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int out_i(int reg, int half) { return 4 * reg + half; }
};
