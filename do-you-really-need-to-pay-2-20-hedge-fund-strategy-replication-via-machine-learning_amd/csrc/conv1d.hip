// Direct causal 1-D convolution for the temporal-conv critic (K14): forward, input gradient and weight
// gradient on the matrix cores, with no unfolded (B, T, k C) tensor in HBM.
//
// Activations are row-major (B, T, C) in bf16 or fp32, seen as M = B T flattened rows; the master kernel
// is fp32 (k, C_in, C_out).  Tap j pairs with the time offset s_j = (k - 1 - j) dil (im2col_causal's
// column-block order).
//
// conv1d_tap_kernel (forward and input gradient: one kernel, the row shift's sign and the weight strides
// differ):  out[r, n] = sum_j sum_c in[r + dir s_j, c] B_j[c, n]  with
//   forward  dir = -1, B_j[c, n] = W[j, c, n], tap j of row (b, t) exists for t - s_j >= 0
//   dgrad    dir = +1, B_j[c, n] = W[j, n, c], tap j of row (b, t) exists for t + s_j <  T
// A persistent workgroup builds the weight operand of every tap once in LDS, already in MFMA fragment
// order (bf16: the 8 values of a lane contiguous, one ds_read_b128 per fragment; fp32: [c][n], the
// 32x32x2 B fragment is a row), then walks row tiles of 64 or 128 rows.  Per tile it stages the rows
// r0 - halo .. r0 + R (forward; dgrad: r0 .. r0 + R + halo; halo = the largest s_j below T) once in LDS
// and every tap reads that image at its own row offset.  Rows outside [0, M) are staged as zeros and
// never addressed.  A tile usually spans several samples: the lane that owns output row r = (b, t)
// replaces its A fragment of tap j by zeros when the tap's source time lies outside [0, T) of sample b,
// so a neighbouring sample's rows, although staged, never reach a product.  A halo too large for LDS
// beside the weights (a long dilation on a long window) is staged per tap instead, R rows at a time.
//   bf16: v_mfma_f32_32x32x16_bf16, fp32 accumulation.
//   fp32: v_mfma_f32_32x32x2_f32, the exact fp32 MFMA (an fmaf chain per output, as widef_kernel).
//
// conv1d_wgrad_kernel:  gW[j, i, o] += sum_r [t(r) >= s_j] x[r - s_j, i] dz[r, o],  gb[o] += sum_r dz[r, o].
// The reduction runs over rows, so both operands are staged TRANSPOSED ([feature][row], 32-row chunks) as
// wgrad_f32s_kernel (gemm.hip) does: grid (row range, tap); the tap's shifted, masked rows of x are
// read straight from global memory while staging (the shift costs nothing there, and the three taps' reads
// of one row meet in L2).  fp32 operands are split exactly into three bf16 planes and the six products
// with terms >= 2^-24 run on the bf16 MFMA (the project's three-term split); bf16 operands are one plane.
// The bias gradient is summed by the threads that stage dz (tap k - 1's workgroups).  Every workgroup
// writes its own slab; launch_split_reduce adds the slabs in a fixed order: no atomics, bitwise
// repeatable, independent of the stream.
#include <algorithm>

#include "kernels.h"
#include "mfma.h"

namespace hfrep {
namespace {

constexpr int CV_LDS = 160 * 1024;  // LDS per workgroup (one CU's whole LDS)
constexpr int CV_CMAX = 128;        // channels: up to four 32-wide MFMA tiles
constexpr int CV_KMAX = 8;          // taps
constexpr int CV_SU = 8;            // staging: vector loads in flight per thread

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// per-dtype geometry of the staged row tile and the weight image
template <typename T> struct CvGeo;
template <> struct CvGeo<float> {
  typedef f32x4 vec;
  static constexpr int KS = 2;
  __host__ __device__ static int pitch(int C) { return C + 1; }  // odd: the 32 rows of a fragment read hit 32 banks
  __host__ __device__ static int ksteps(int C) { return C / 2; }
  static size_t wbytes(int k, int C, int N, int) { return ((size_t)k * C * N * 4 + 15) / 16 * 16; }
};
template <> struct CvGeo<bf16_t> {
  typedef u32x2 vec;
  static constexpr int KS = 16;
  __host__ __device__ static int pitch(int C) { return (C + 15) / 16 * 16 + 8; }  // 16-B aligned rows, banks spread
  __host__ __device__ static int ksteps(int C) { return (C + 15) / 16; }
  static size_t wbytes(int k, int C, int, int NT) { return (size_t)k * ksteps(C) * NT * 64 * 8 * 2; }
};

// ---------------------------------------------------------------------------------------------
// forward / input gradient
// ---------------------------------------------------------------------------------------------
template <typename T, int NT, int RT>
__global__ void __launch_bounds__(256)
conv1d_tap_kernel(const T* __restrict__ in, const float* __restrict__ W, const float* __restrict__ bias,
                  T* __restrict__ out, int M, int Tn, int C, int N, int k, int dil, int dir, int sc, int sn, int act,
                  int j0, int jmin, int j1, int accum, int per_tap, int wbytes) {
  using P = MF<T>;
  using G = CvGeo<T>;
  using VT = typename G::vec;  // four elements
  constexpr int R = 32 * RT;
  constexpr int TPW = (NT * RT + 3) / 4;  // output tiles per wave
  constexpr int NSTR = 4 / RT;            // column-tile stride between a wave's tiles
  extern __shared__ __attribute__((aligned(16))) unsigned char cv_smem[];
  T* wimg = reinterpret_cast<T*>(cv_smem);
  T* tile = reinterpret_cast<T*>(cv_smem + wbytes);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, cl = lane & 31;
  const int pitch = G::pitch(C), nks = G::ksteps(C), C4 = C / 4;
  const int halo = (k - 1 - jmin) * dil;  // the largest shift below Tn
  const int wrows = per_tap ? R : R + halo;

  // ---- weight image of the taps j0 .. j1 of this launch (jmin: the first of them that can contribute),
  //      once per workgroup ----
  if constexpr (sizeof(T) == 4) {
    const int CN = C * N;
    for (int e = tid; e < (j1 - j0) * CN; e += 256) {
      const int j = j0 + e / CN, rem = e % CN, c = rem / N, n = rem - c * N;
      wimg[e] = W[(size_t)j * CN + (size_t)c * sc + (size_t)n * sn];
    }
  } else {
    const int CN = C * N;
    for (int e = tid; e < (j1 - j0) * nks * NT * 64; e += 256) {
      const int l = e & 63;
      int rest = e >> 6;
      const int nt = rest % NT;
      rest /= NT;
      const int ks = rest % nks, j = j0 + rest / nks;
      const int n = 32 * nt + (l & 31), c0 = 16 * ks + 8 * (l >> 5);
      bf16x8 f;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int c = c0 + q;
        const float v = (c < C && n < N) ? W[(size_t)j * CN + (size_t)c * sc + (size_t)n * sn] : 0.f;
        f[q] = (short)f2bf(v);
      }
      reinterpret_cast<bf16x8*>(wimg)[e] = f;
    }
  }
  // the tile's pad columns (bf16: C .. ceil16(C)) are read by the last k step and never staged: zero once
  for (int e = tid; e < wrows * pitch; e += 256) tile[e] = (T)0;
  __syncthreads();

  const int rt = w % RT;
  int ntq[TPW];
#pragma unroll
  for (int q = 0; q < TPW; ++q) ntq[q] = w / RT + NSTR * q;

  const int ntiles = (M + R - 1) / R;
  for (int tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const int r0 = tl * R;
    const int t = (r0 + 32 * rt + cl) % Tn;  // this lane's output row's time step
    f32x16 acc[TPW];
#pragma unroll
    for (int q = 0; q < TPW; ++q) acc[q] = zero16();
    const int ngroups = per_tap ? j1 - jmin : 1;
    for (int g = 0; g < ngroups; ++g) {
      const int jlo = jmin + g, jhi = per_tap ? jlo + 1 : j1;
      // first staged row: the tap's own source rows (per tap), else the tile with its halo
      const int base = per_tap ? r0 + dir * (k - 1 - jlo) * dil : (dir < 0 ? r0 - halo : r0);
      // eight vector loads in flight per thread, then their LDS writes (a load per write exposed the whole
      // memory latency seven times per 64-row tile)
      const int nvec = wrows * C4;
      for (int e0 = tid; e0 < nvec; e0 += 256 * CV_SU) {
        VT v[CV_SU];
#pragma unroll
        for (int u = 0; u < CV_SU; ++u) {
          const int e = e0 + 256 * u, row = e / C4, c4 = e - row * C4, gr = base + row;
          v[u] = VT{};
          if (e < nvec && gr >= 0 && gr < M)  // C % 4 == 0: a vector of four elements is as aligned as the base
            v[u] = *reinterpret_cast<const VT*>(in + (size_t)gr * C + 4 * c4);
        }
#pragma unroll
        for (int u = 0; u < CV_SU; ++u) {
          const int e = e0 + 256 * u, row = e / C4, c4 = e - row * C4;
          if (e < nvec) {
            if constexpr (sizeof(T) == 4) {
              float* d = tile + row * pitch + 4 * c4;  // (odd pitch: four scalar writes)
              d[0] = v[u][0]; d[1] = v[u][1]; d[2] = v[u][2]; d[3] = v[u][3];
            } else {
              *reinterpret_cast<VT*>(tile + row * pitch + 4 * c4) = v[u];
            }
          }
        }
      }
      __syncthreads();
      for (int j = jlo; j < jhi; ++j) {
        const int s = (k - 1 - j) * dil;
        const bool valid = dir < 0 ? t >= s : t + s < Tn;  // the tap's source time is inside this row's sample
        const T* arow = tile + (32 * rt + cl + (r0 + dir * s - base)) * pitch;
#pragma unroll 4
        for (int ks = 0; ks < nks; ++ks) {
          typename P::frag a = P::lda(arow, ks, lane);
          if (!valid) a = P::zero();
#pragma unroll
          for (int q = 0; q < TPW; ++q) {
            const int nt = min(ntq[q], NT - 1);  // (a wave with no tile left repeats the last one and stores nothing)
            typename P::frag b;
            if constexpr (sizeof(T) == 4)
              b = wimg[((j - j0) * C + 2 * ks + h) * N + min(32 * nt + cl, N - 1)];  // columns past N: any value, never stored
            else
              b = reinterpret_cast<const bf16x8*>(wimg)[(((j - j0) * nks + ks) * NT + nt) * 64 + lane];
            acc[q] = P::mma(a, b, acc[q]);
          }
        }
      }
      __syncthreads();
    }
    // the accumulators are read behind the loop exits, where the hazard recognizer does not count the
    // MFMA write -> read wait states (tests/test_isa_hazards.py): 24 explicit ones per tile (the 16-pass
    // fp32 MFMA needs 18)
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
      const int col = 32 * ntq[q] + cl;
      if (ntq[q] < NT && col < N) {
        const float bv = bias ? bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = r0 + 32 * rt + acc32_row(r, lane);
          if (row < M) {
            T* o = out + (size_t)row * N + col;
            const float prev = accum ? ld_f(o) : 0.f;  // (the earlier taps' launch: fp32 only)
            st_f(o, act_f(act, acc[q][r] + prev + bv));
          }
        }
      }
    }
  }
}

struct TapPlan {
  int NT, RT, per_tap;
  size_t wbytes, smem;
  bool ok;
};

// taps j0 .. j1 of one launch, jmin the first that can contribute; C: the summed channel count, N: the output's
template <typename T>
TapPlan tap_plan(int M, int C, int N, int ntaps, int halo) {
  using G = CvGeo<T>;
  TapPlan p{};
  p.NT = (N + 31) / 32;
  p.wbytes = G::wbytes(ntaps, C, N, p.NT);
  const size_t rowb = (size_t)G::pitch(C) * sizeof(T);
  // 128-row tiles (a wave owns a row tile and every column tile: the most reuse of its A fragments) when
  // they fit and still give every CU a tile; 64-row tiles otherwise
  const bool many = (M + 127) / 128 >= device_cu_count();
  const int order[2] = {many ? 4 : 2, many ? 2 : 4};
  p.ok = false;
  for (int per_tap = 0; per_tap < 2 && !p.ok; ++per_tap)
    for (int o = 0; o < 2 && !p.ok; ++o) {
      const int rt = order[o], rows = 32 * rt + (per_tap ? 0 : halo);
      if (p.wbytes + (size_t)rows * rowb <= (size_t)CV_LDS) {
        p.RT = rt;
        p.per_tap = per_tap;
        p.smem = p.wbytes + (size_t)rows * rowb;
        p.ok = true;
      }
    }
  return p;
}

// the most taps whose weight operand fits in LDS beside a 64-row tile (0: not even one)
template <typename T>
int taps_per_launch(int C, int N, int k) {
  using G = CvGeo<T>;
  int n = k;
  while (n > 0 && G::wbytes(n, C, N, (N + 31) / 32) + (size_t)64 * G::pitch(C) * sizeof(T) > (size_t)CV_LDS) --n;
  return n;
}

template <typename T, int NT, int RT>
void launch_tap_inst(const TapPlan& p, const T* in, const float* W, const float* bias, T* out, int M, int Tn, int C, int N,
                     int k, int dil, int dir, int sc, int sn, int act, int j0, int jmin, int j1, int accum, hipStream_t s) {
  static bool attr = false;  // (per instantiation: more than 64 KiB of dynamic LDS needs the attribute)
  auto kern = conv1d_tap_kernel<T, NT, RT>;
  if (!attr) {
    HFREP_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        CV_LDS));
    attr = true;
  }
  const int ntiles = (M + 32 * RT - 1) / (32 * RT);
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, (size_t)CV_LDS / p.smem));
  const int grid = std::max(1, std::min(ntiles, device_cu_count() * per_cu));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), p.smem, s, in, W, bias, out, M, Tn, C, N, k, dil, dir, sc, sn, act,
                     j0, jmin, j1, accum, p.per_tap, (int)p.wbytes);
  HFREP_CHECK_HIP(hipGetLastError());
}

// All k taps in one launch where their weight operand fits in LDS (every zoo shape but fp32 C = 100 with
// k = 4); otherwise the taps go in groups, last group last: an earlier launch stores its partial sums raw,
// the next adds them to its own, the last applies bias and activation.  fp32 only, so the partial sums lose
// nothing (a bf16 shape whose weight operand does not fit is declined).
template <typename T>
bool launch_tap(const T* in, const float* W, const float* bias, T* out, int M, int Tn, int C, int N, int k, int dil,
                int dir, int sc, int sn, int act, hipStream_t s) {
  const int per = taps_per_launch<T>(C, N, k);
  if (per < 1 || (per < k && sizeof(T) != 4)) return false;
  int jmin = 0;  // the first tap whose shift is below Tn (the earlier ones never contribute)
  while (jmin < k - 1 && (int64_t)(k - 1 - jmin) * dil >= Tn) ++jmin;
  int accum = 0;
  for (int j1 = jmin + (k - jmin - 1) % per + 1, j0 = jmin; j0 < k; j0 = j1, j1 += per) {
    const bool last = j1 == k;
    const TapPlan p = tap_plan<T>(M, C, N, j1 - j0, (k - 1 - j0) * dil);
    if (!p.ok) return false;
    const float* b = last ? bias : nullptr;
    const int a = last ? act : 0;
#define HFREP_CV_TAP(NT_, RT_)                                                                                      \
  case NT_ * 8 + RT_:                                                                                               \
    launch_tap_inst<T, NT_, RT_>(p, in, W, b, out, M, Tn, C, N, k, dil, dir, sc, sn, a, j0, j0, j1, accum, s);     \
    break;
    switch (p.NT * 8 + p.RT) {
      HFREP_CV_TAP(1, 2) HFREP_CV_TAP(2, 2) HFREP_CV_TAP(3, 2) HFREP_CV_TAP(4, 2)
      HFREP_CV_TAP(1, 4) HFREP_CV_TAP(2, 4) HFREP_CV_TAP(3, 4) HFREP_CV_TAP(4, 4)
      default: return false;
    }
#undef HFREP_CV_TAP
    accum = 1;
  }
  return true;
}

// ---------------------------------------------------------------------------------------------
// weight gradient
// ---------------------------------------------------------------------------------------------
constexpr int CWR = 32;       // rows per chunk
constexpr int CWQ = CWR + 8;  // image row pitch (bf16): 80 bytes

// exact three-way split of 8 fp32 values into bf16 planes (hi / mid / lo: 8 mantissa bits each)
__device__ __forceinline__ void cv_split8(const float (&v)[8], bf16x8& hi, bf16x8& mi, bf16x8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float a = v[j];  // (a scalar copy first: tests/test_isa_hazards.py bit_cast lint)
    const uint32_t u = __builtin_bit_cast(uint32_t, a), hb = u & 0xffff0000u;
    const float r1 = a - __builtin_bit_cast(float, hb);
    const uint32_t m = __builtin_bit_cast(uint32_t, r1) & 0xffff0000u;
    const float r2 = r1 - __builtin_bit_cast(float, m);
    hi[j] = (short)(hb >> 16);
    mi[j] = (short)(m >> 16);
    lo[j] = (short)(__builtin_bit_cast(uint32_t, r2) >> 16);
  }
}

template <typename T, int NI, int NJ>
__global__ void __launch_bounds__(256)
conv1d_wgrad_kernel(const T* __restrict__ X, const T* __restrict__ D, float* __restrict__ slab, int M, int Tn, int K,
                    int N, int k, int dil, int rows_per_split, int has_bias) {
  constexpr int NP = sizeof(T) == 4 ? 3 : 1;             // bf16 planes per operand
  constexpr int PX = NI * 32 * CWQ, PD = NJ * 32 * CWQ;  // plane sizes (bf16)
  constexpr int TX = (NI + 1) / 2, TD = (NJ + 1) / 2;    // (feature, 8-row group) tasks per thread
  constexpr int TPW = (NI * NJ + 3) / 4;                 // output tiles per wave
  __shared__ __attribute__((aligned(16))) bf16_t img[NP * PX + NP * PD];
  bf16_t* ix = img;
  bf16_t* id = img + NP * PX;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, cl = lane & 31;
  const int j = blockIdx.y;
  const int64_t s64 = (int64_t)(k - 1 - j) * dil;
  const int s = s64 < Tn ? (int)s64 : Tn;  // (Tn or more: the tap never contributes)
  const int mb = blockIdx.x * rows_per_split;
  const int me = s < Tn ? min(M, mb + rows_per_split) : mb;  // a tap that never contributes: a slab of zeros
  const bool do_bias = has_bias && j == k - 1;               // (s == 0: that tap sees every row)
  for (int e = tid; e < (NP * PX + NP * PD) / 8; e += 256) reinterpret_cast<bf16x8*>(img)[e] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
  f32x16 acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) acc[t] = zero16();
  float vx[TX][8], vd[TD][8], bsum[TD];
#pragma unroll
  for (int q = 0; q < TD; ++q) bsum[q] = 0.f;
  auto load = [&](int m0) {
#pragma unroll
    for (int q = 0; q < TX; ++q) {
      const int e = tid + 256 * q, i = e % K, rg = e / K;
      const int rb = m0 + 8 * rg;
      int t = rb % Tn;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int r = rb + jj;
        // row (b, t) takes x[b, t - s]: inside the sample for t >= s (so r - s >= 0 too)
        vx[q][jj] = (rg < 4 && r < me && t >= s) ? ld_f(X + (size_t)(r - s) * K + i) : 0.f;
        if (++t == Tn) t = 0;
      }
    }
#pragma unroll
    for (int q = 0; q < TD; ++q) {
      const int e = tid + 256 * q, j0 = e % N, rg = e / N;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int r = m0 + 8 * rg + jj;
        vd[q][jj] = (rg < 4 && r < me) ? ld_f(D + (size_t)r * N + j0) : 0.f;
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int q = 0; q < TX; ++q) {
      const int e = tid + 256 * q, i = e % K, rg = e / K;
      if (rg < 4) {
        const int o = i * CWQ + 8 * rg;
        if constexpr (NP == 3) {
          bf16x8 a, b, c;
          cv_split8(vx[q], a, b, c);
          *reinterpret_cast<bf16x8*>(ix + o) = a;
          *reinterpret_cast<bf16x8*>(ix + PX + o) = b;
          *reinterpret_cast<bf16x8*>(ix + 2 * PX + o) = c;
        } else {
          bf16x8 a;
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) a[jj] = (short)f2bf(vx[q][jj]);  // (bf16 values: exact)
          *reinterpret_cast<bf16x8*>(ix + o) = a;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < TD; ++q) {
      const int e = tid + 256 * q, j0 = e % N, rg = e / N;
      if (rg < 4) {
        const int o = j0 * CWQ + 8 * rg;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) bsum[q] += vd[q][jj];
        if constexpr (NP == 3) {
          bf16x8 a, b, c;
          cv_split8(vd[q], a, b, c);
          *reinterpret_cast<bf16x8*>(id + o) = a;
          *reinterpret_cast<bf16x8*>(id + PD + o) = b;
          *reinterpret_cast<bf16x8*>(id + 2 * PD + o) = c;
        } else {
          bf16x8 a;
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) a[jj] = (short)f2bf(vd[q][jj]);
          *reinterpret_cast<bf16x8*>(id + o) = a;
        }
      }
    }
  };
  __syncthreads();
  if (mb < me) load(mb);
  for (int m0 = mb; m0 < me; m0 += CWR) {
    stage();
    __syncthreads();
    load(m0 + CWR);  // the next chunk's loads fly during the MFMAs (past me: zeros, no access)
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int tile = w + 4 * t;
      if (tile < NI * NJ) {
        const int ti = tile / NJ, tj = tile - ti * NJ;
#pragma unroll
        for (int ks = 0; ks < CWR / 16; ++ks) {
          const int ao = (32 * ti + cl) * CWQ + 16 * ks + 8 * h, bo = (32 * tj + cl) * CWQ + 16 * ks + 8 * h;
          const bf16x8 ah = *reinterpret_cast<const bf16x8*>(ix + ao);
          const bf16x8 bh = *reinterpret_cast<const bf16x8*>(id + bo);
          if constexpr (NP == 3) {
            const bf16x8 am = *reinterpret_cast<const bf16x8*>(ix + PX + ao);
            const bf16x8 al = *reinterpret_cast<const bf16x8*>(ix + 2 * PX + ao);
            const bf16x8 bm = *reinterpret_cast<const bf16x8*>(id + PD + bo);
            const bf16x8 bl = *reinterpret_cast<const bf16x8*>(id + 2 * PD + bo);
            acc[t] = MF<bf16_t>::mma(am, bm, acc[t]);
            acc[t] = MF<bf16_t>::mma(al, bh, acc[t]);
            acc[t] = MF<bf16_t>::mma(ah, bl, acc[t]);
            acc[t] = MF<bf16_t>::mma(am, bh, acc[t]);
            acc[t] = MF<bf16_t>::mma(ah, bm, acc[t]);
          }
          acc[t] = MF<bf16_t>::mma(ah, bh, acc[t]);
        }
      }
    }
    // accumulators are read after the loop, behind the wave-uniform tile branch and the loop exit: 16
    // explicit wait states after each chunk's MFMAs (as wgrad_f32s_kernel, tests/test_isa_hazards.py)
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
  }
  const int KN = K * N;
  float* out = slab + (size_t)blockIdx.x * ((size_t)k * KN + (has_bias ? N : 0));
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int tile = w + 4 * t;
    if (tile < NI * NJ) {
      const int ti = tile / NJ, tj = tile - ti * NJ, col = 32 * tj + cl;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * ti + acc32_row(r, lane);
        if (row < K && col < N) out[(size_t)j * KN + (size_t)row * N + col] = acc[t][r];
      }
    }
  }
  if (do_bias) {  // (workgroup-uniform) the four row groups of every dz column, summed in a fixed order
    float* red = reinterpret_cast<float*>(img);  // [4][N] floats: the images are dead (the loop's last barrier)
#pragma unroll
    for (int q = 0; q < TD; ++q) {
      const int e = tid + 256 * q, j0 = e % N, rg = e / N;
      if (rg < 4) red[rg * N + j0] = bsum[q];
    }
    __syncthreads();
    if (tid < N) out[(size_t)k * KN + tid] = (red[tid] + red[N + tid]) + (red[2 * N + tid] + red[3 * N + tid]);
  }
}

int cv_wgrad_splits(int M, int k) {
  const int want = (M + 1023) / 1024;  // >= 32 chunks per workgroup
  return std::max(1, std::min(want, std::max(1, device_cu_count() * 2 / k)));
}
int cv_wgrad_rps(int M, int k) {
  const int P = cv_wgrad_splits(M, k);
  return ((M + P - 1) / P + CWR - 1) / CWR * CWR;
}

template <typename T>
bool launch_cv_wgrad(const T* X, const T* D, float* ws, int M, int Tn, int K, int N, int k, int dil, int has_bias,
                     hipStream_t s) {
  const int rps = cv_wgrad_rps(M, k), z = (M + rps - 1) / rps;
  const int ni = (K + 31) / 32, nj = (N + 31) / 32;
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(z, k), dim3(256), 0, s, X, D, ws, M, Tn, K, N, k, dil, rps, has_bias);
    HFREP_CHECK_HIP(hipGetLastError());
  };
  if (nj != 4) return false;
  switch (ni) {
    case 1: go(conv1d_wgrad_kernel<T, 1, 4>); break;
    case 2: go(conv1d_wgrad_kernel<T, 2, 4>); break;
    case 3: go(conv1d_wgrad_kernel<T, 3, 4>); break;
    case 4: go(conv1d_wgrad_kernel<T, 4, 4>); break;
    default: return false;
  }
  return true;
}

template <typename T>
bool cv_supported(int Cin, int Cout, int k) {
  if (Cin < 4 || Cin > CV_CMAX || Cin % 4 || Cout <= 96 || Cout > CV_CMAX || Cout % 4 || k < 1 || k > CV_KMAX) return false;
  // the weight operand beside a 64-row tile, in both directions: all taps in bf16, at least one in fp32 (the
  // halo never decides: a long one is staged per tap)
  const int need = sizeof(T) == 4 ? 1 : k;
  return taps_per_launch<T>(Cin, Cout, k) >= need && taps_per_launch<T>(Cout, Cin, k) >= need;
}

}  // namespace

bool conv1d_supported(int dt, int Cin, int Cout, int k, int dil) {
  if (dil < 1) return false;
  return dt == DT_BF16 ? cv_supported<bf16_t>(Cin, Cout, k) : cv_supported<float>(Cin, Cout, k);
}

bool launch_conv1d_fwd(int dt, const void* x, const float* W, const float* bias, void* y, int B, int Tn, int Cin,
                       int Cout, int k, int dil, int act, hipStream_t s) {
  if (!conv1d_supported(dt, Cin, Cout, k, dil)) return false;
  const int64_t M64 = (int64_t)B * Tn;
  if (M64 <= 0) return true;
  if (M64 > (int64_t)INT32_MAX - 1024) return false;
  const int M = (int)M64, d = std::min(dil, Tn);  // a shift of Tn or more never contributes: any such dil is Tn
  return dt == DT_BF16 ? launch_tap<bf16_t>((const bf16_t*)x, W, bias, (bf16_t*)y, M, Tn, Cin, Cout, k, d, -1, Cout, 1, act, s)
                       : launch_tap<float>((const float*)x, W, bias, (float*)y, M, Tn, Cin, Cout, k, d, -1, Cout, 1, act, s);
}

bool launch_conv1d_dgrad(int dt, const void* dz, const float* W, void* dx, int B, int Tn, int Cin, int Cout, int k,
                         int dil, hipStream_t s) {
  if (!conv1d_supported(dt, Cin, Cout, k, dil)) return false;
  const int64_t M64 = (int64_t)B * Tn;
  if (M64 <= 0) return true;
  if (M64 > (int64_t)INT32_MAX - 1024) return false;
  const int M = (int)M64, d = std::min(dil, Tn);
  // B_j[c = o][n = i] = W[j][i][o]
  return dt == DT_BF16 ? launch_tap<bf16_t>((const bf16_t*)dz, W, nullptr, (bf16_t*)dx, M, Tn, Cout, Cin, k, d, +1, 1, Cout, 0, s)
                       : launch_tap<float>((const float*)dz, W, nullptr, (float*)dx, M, Tn, Cout, Cin, k, d, +1, 1, Cout, 0, s);
}

size_t conv1d_wgrad_workspace_floats(int B, int Tn, int Cin, int Cout, int k, bool has_bias) {
  const int64_t M = (int64_t)B * Tn;
  if (M <= 0 || M > (int64_t)INT32_MAX - 1024) return 0;
  const int rps = cv_wgrad_rps((int)M, k), z = ((int)M + rps - 1) / rps;
  return (size_t)z * ((size_t)k * Cin * Cout + (has_bias ? Cout : 0));
}

bool launch_conv1d_wgrad(int dt, const void* x, const void* dz, float* gW, float* gb, int B, int Tn, int Cin, int Cout,
                         int k, int dil, float* ws, hipStream_t s) {
  if (!conv1d_supported(dt, Cin, Cout, k, dil)) return false;
  const int64_t M64 = (int64_t)B * Tn;
  if (M64 <= 0) return true;
  if (M64 > (int64_t)INT32_MAX - 1024) return false;
  const int M = (int)M64, d = std::min(dil, Tn), has_bias = gb != nullptr;
  const bool ok = dt == DT_BF16 ? launch_cv_wgrad<bf16_t>((const bf16_t*)x, (const bf16_t*)dz, ws, M, Tn, Cin, Cout, k, d, has_bias, s)
                                : launch_cv_wgrad<float>((const float*)x, (const float*)dz, ws, M, Tn, Cin, Cout, k, d, has_bias, s);
  if (!ok) return false;
  const int rps = cv_wgrad_rps(M, k), z = (M + rps - 1) / rps;
  launch_split_reduce(ws, gW, gb, z, k * Cin * Cout, has_bias ? Cout : 0, s);
  return true;
}

}  // namespace hfrep
