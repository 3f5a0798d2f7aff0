// fp32 LSTM gradient GEMMs (gfx950): the fused weight gradients -- exact fp32 (lstmf_wgrad_kernel) and the
// three-term bf16 split as a column pair, a column quad and with MFMA / staging wave roles -- and the
// input gradients dX = dZ W^T (lstmf_dgrad_kernel exact, lstmf_dgrad_s4_kernel split, lstmf_dgrad_roles_kernel
// the same split with MFMA / staging wave roles), with their launchers.  The recurrent kernels (forwards, BPTTs, tangent reverses) are in lstm_f32.hip; what both
// files share is in lstmf_dev.h.
#include "lstmf_dev.h"

#include <stdexcept>
#include <type_traits>

namespace hfrep {

// ==========================================================================================
// fused fp32 LSTM weight gradients
// ==========================================================================================
// slab[z] ((K + H + 1) x 4H) = sum over workgroup z's rows m of [x_m | h_{m-1} | 1]^T dz_m, plus the
// tangent segment [xd_m | hd_{m-1} | 0]^T dzd_m when given; one fixed-order reduce folds the slabs
// into gW / gU / gb (launch_lstm_wgrad2_reduce).  The v1 fp32 path ran one tiled GEMM per product
// (X^T dZ, H^T dZ, Xd^T dZd, Hd^T dZd: each re-reading dZ, ~35 TF/s, profiles/r02_fp32): here every
// (row chunk) is staged once and feeds all products.
//
// 8 waves (2 per SIMD), 16-row chunks = four 16x16x4 k-steps; output tiles 16 x 16: wave w owns the
// full i range of column tiles 3 w .. 3 w + 2 plus i-tiles 2 w, 2 w + 1 of the 25th column tile,
// i.e. 3 NI + 2 accumulators (K = 100: 41 x 4 AGPRs), the same MFMA count on every wave.
// Chunks are double-buffered in LDS through a register prefetch of the next chunk.
constexpr int WF_R = 16, WF_LA = 272, WF_LD = 400;  // row strides = 16 mod 64 dwords: conflict-free b32 reads
template <int KX>
struct WFGeo {
  static constexpr int KR = KX + FH + 1;
  static constexpr int NI = (KR + 15) / 16;
  static_assert(NI <= 16 && 16 * 16 <= WF_LA, "wgrad i tiles");
  static constexpr int NX4 = WF_R * KX / 4, NH4 = WF_R * FH / 4, ND4 = WF_R * FG / 4;
  static constexpr int JX = (NX4 + 511) / 512, JH = (NH4 + 511) / 512, JD = (ND4 + 511) / 512;
};

template <int KX, int XR = KX>  // XR: X row stride in floats (35: a 36-column image, column 35 zero)
__global__ void __launch_bounds__(512)
lstmf_wgrad_kernel(const float* __restrict__ X, const float* __restrict__ Hs, const float* __restrict__ D,
                   const float* __restrict__ Xd, const float* __restrict__ Hds, const float* __restrict__ Dd,
                   float* __restrict__ slab, int M, int Tn, int rows_per_wg) {
  using WG = WFGeo<KX>;
  constexpr int NI = WG::NI, KR = WG::KR;
  __shared__ __attribute__((aligned(16))) float As[2][WF_R * WF_LA];
  __shared__ __attribute__((aligned(16))) float Ds[2][WF_R * WF_LD];
  __shared__ __attribute__((aligned(16))) float trash4[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  const int mb = blockIdx.x * rows_per_wg, me = min(M, mb + rows_per_wg);
  for (int i = tid; i < 2 * WF_R * WF_LA; i += 512) (&As[0][0])[i] = 0.f;

  f32x4 acc[NI][3], accx[2];
#pragma unroll
  for (int it = 0; it < NI; ++it)
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) acc[it][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
  accx[0] = accx[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ie0 = min(2 * w, 15), ie1 = min(2 * w + 1, 15);  // i tiles >= NI read LDS zeros

  // per-thread chunk loads: X (JX), H_{m-1} (JH), D (JD) float4s
  f32x4 vx[WG::JX], vh[WG::JH], vd[WG::JD];
  for (int seg = 0; seg < (Xd ? 2 : 1); ++seg) {
    const float* Xs = seg ? Xd : X;
    const float* Hq = seg ? Hds : Hs;
    const float* Dq = seg ? Dd : D;
    // descriptors based at this workgroup's first row (row mb - 1 for the shifted H): the byte
    // offsets stay 32-bit however large M is (a whole-tensor base overflowed past 1.34 M rows of dZ)
    const int hb = mb > 0 ? mb - 1 : 0, nr = me > mb ? me - mb : 0;
    const rsrc_t rx = make_rsrc(Xs + (size_t)mb * XR, nr * XR * 4);
    const rsrc_t rh = make_rsrc(Hq + (size_t)hb * FH, (nr ? me - hb : 0) * FH * 4);
    const rsrc_t rd = make_rsrc(Dq + (size_t)mb * FG, nr * FG * 4);
    auto load = [&](int m0) {
#pragma unroll
      for (int j = 0; j < WG::JX; ++j) {
        const int e = tid + 512 * j, r = e / (KX / 4), c = e - r * (KX / 4);
        const bool ok = e < WG::NX4 && m0 + r < me;
        vx[j] = ldx4<XR>(rx, ok ? ((m0 - mb + r) * XR + 4 * c) * 4 : kOOB, 0, 4 * c);
      }
#pragma unroll
      for (int j = 0; j < WG::JH; ++j) {
        const int e = tid + 512 * j, r = e / (FH / 4), c = e - r * (FH / 4);
        const int m = m0 + r;
        const bool ok = e < WG::NH4 && m < me && (m % Tn) != 0;  // h_{-1} = 0 at t = 0
        vh[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rh, ok ? ((m - 1 - hb) * FH + 4 * c) * 4 : kOOB, 0, 0));
      }
#pragma unroll
      for (int j = 0; j < WG::JD; ++j) {
        const int e = tid + 512 * j, r = e / (FG / 4), c = e - r * (FG / 4);
        const bool ok = e < WG::ND4 && m0 + r < me;
        vd[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rd, ok ? ((m0 - mb + r) * FG + 4 * c) * 4 : kOOB, 0, 0));
      }
    };
    auto to_lds = [&](int buf) {
#pragma unroll
      for (int j = 0; j < WG::JX; ++j) {
        const int e = tid + 512 * j, r = e / (KX / 4), c = e - r * (KX / 4);
        *reinterpret_cast<f32x4*>(e < WG::NX4 ? &As[buf][r * WF_LA + 4 * c] : trash4) = vx[j];
      }
#pragma unroll
      for (int j = 0; j < WG::JH; ++j) {
        const int e = tid + 512 * j, r = e / (FH / 4), c = e - r * (FH / 4);
        *reinterpret_cast<f32x4*>(e < WG::NH4 ? &As[buf][r * WF_LA + KX + 4 * c] : trash4) = vh[j];
      }
#pragma unroll
      for (int j = 0; j < WG::JD; ++j) {
        const int e = tid + 512 * j, r = e / (FG / 4), c = e - r * (FG / 4);
        *reinterpret_cast<f32x4*>(e < WG::ND4 ? &Ds[buf][r * WF_LD + 4 * c] : trash4) = vd[j];
      }
    };
    __syncthreads();  // (previous segment's reads done)
    if (tid < 2 * WF_R) As[tid >> 4][(tid & 15) * WF_LA + KR - 1] = seg ? 0.f : 1.f;  // the bias column
    if (mb < me) {
      load(mb);
      to_lds(0);
    }
    __syncthreads();
    int buf = 0;
    for (int m0 = mb; m0 < me; m0 += WF_R) {
      const bool more = m0 + WF_R < me;
      if (more) load(m0 + WF_R);
      const float* A_ = As[buf];
      const float* D_ = Ds[buf];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const float* ar = A_ + (4 * ks + g) * WF_LA + c16;
        const float* dr = D_ + (4 * ks + g) * WF_LD + c16;
        float a[NI], b[3];
#pragma unroll
        for (int it = 0; it < NI; ++it) a[it] = ar[16 * it];
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) b[jj] = dr[16 * (3 * w + jj)];
        const float bx = dr[16 * 24], ax0 = ar[16 * ie0], ax1 = ar[16 * ie1];
#pragma unroll
        for (int it = 0; it < NI; ++it)
#pragma unroll
          for (int jj = 0; jj < 3; ++jj) acc[it][jj] = mma4(a[it], b[jj], acc[it][jj]);
        accx[0] = mma4(ax0, bx, accx[0]);
        accx[1] = mma4(ax1, bx, accx[1]);
      }
      if (more) to_lds(buf ^ 1);
      buf ^= 1;
      __syncthreads();
    }
  }
  // ---- slab store: C[i0 + 4 g + r][j0 + c16] ----
  float* out = slab + (size_t)blockIdx.x * KR * FG;
#pragma unroll
  for (int it = 0; it < NI; ++it)
#pragma unroll
    for (int jj = 0; jj < 3; ++jj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * it + 4 * g + r;
        if (i < KR) out[(size_t)i * FG + 16 * (3 * w + jj) + c16] = acc[it][jj][r];
      }
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int it = 2 * w + e;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * it + 4 * g + r;
      if (it < NI && i < KR) out[(size_t)i * FG + 16 * 24 + c16] = accx[e][r];
    }
  }
}

// ------------------------------------------------------------------------------------------
// fp32 weight gradient on the bf16 matrix pipe: three-term split, six products
// ------------------------------------------------------------------------------------------
// lstmf_wgrad_kernel above runs at ~83 % of the fp32 MFMA rate (64 FLOP/clk/SIMD), which is 1/16 of
// the bf16 rate.  Here every fp32 operand a is split EXACTLY into three bf16 terms by truncation,
// a = h + m + l (h = top 8 significand bits, m = the next 8, l = the last 8: the two subtractions
// are exact), and C += A^T D is accumulated as hh + hm + mh + mm + hl + lh on
// v_mfma_f32_16x16x32_bf16 (bf16 x bf16 products are exact in fp32, accumulation in fp32).  The
// dropped terms ml, lm, ll are <= 2^-24 |a b| -- the rounding error of one fp32 product -- so the
// result matches the exact-fp32 kernel to fp32 reduction noise (test_lstmf_wgrad_split_*), at 6/16
// of its matrix-pipe time.
//
// Work split: a workgroup PAIR shares a row range z and splits the 400 gate columns in two parts of
// 208 (13 j-tiles; the second part 192 + 1 zero tile); the pair sits on one XCD (blocks b, b + 8), so
// the A rows [x | h_{t-1} | 1] both read come from the same L2.  Per 32-row chunk the workgroup
// stages the three bf16 planes of A (32 x 208) and of its D part (32 x 208) in LDS, double-buffered
// (2 x 78 KB): the next chunk's fp32 rows are loaded into registers before the MFMAs
// and split into the other buffer after them, one barrier per chunk.  MFMA operands come from
// ds_read_b64_tr_b16 (row-major image, hardware transpose: lane 4q + p of a 16-lane group addresses
// row q, columns 4p..4p+3).  8 waves: wave w owns i-tiles [0, NI0) or [NI0, NI) (w >> 2) times a
// group of 4 / 3 / 3 / 3 local j-tiles (reversed for w >= 4 so each SIMD's two waves carry ~equal
// MFMA counts); its B fragments (all three planes of its <= 3 j-tiles) stay in registers for the
// chunk, the A fragments stream: every operand is read from LDS once per wave.  (A three-part
// column split was measured slower: profiles/r02_split.)
constexpr int WS_CA = 208, WS_CD = 208;                   // max image columns (A, D part)
// Row stride of a plane image with `cols` bf16 columns: S dwords with S % 64 == 8 (cf), else packed.
// One ds_read_b64_tr_b16 lane group (32 lanes) reads 8 consecutive chunk rows (tr_frag's row order) x 8
// dwords; at S % 64 == 8 those are the 64 banks once each.  The r02 stride (416 B = 104 dwords) put
// rows r and r + 8 of the old row order on the same banks: 2-way on every operand read
// (SQ_LDS_BANK_CONFLICT ~ 24 % of the q4 kernel's cycles, profiles/r03_split/pmc_summary_v1.txt).
constexpr int ws_row_bytes(int cols, bool cf) {
  const int dw = (cols + 1) / 2;
  return 4 * (cf ? dw + ((8 - dw % 64) + 64) % 64 : (dw + 3) / 4 * 4);
}
// one double-buffered LDS stage: A image (CA columns) + D image (CD columns), three planes each; the
// conflict-free strides where both buffers fit the 160 KiB
template <int CA, int CD>
struct WImg {
  static constexpr bool CF = 2 * 3 * 32 * (ws_row_bytes(CA, true) + ws_row_bytes(CD, true)) <= 160 * 1024;
  static constexpr int ROWA = ws_row_bytes(CA, CF), ROWD = ws_row_bytes(CD, CF);  // bytes per image row
  static constexpr int PLA = 32 * ROWA, PLD = 32 * ROWD;                           // bytes per plane
  static constexpr int IMGD = 3 * PLA;                                             // D image offset
  static constexpr int BUF = 3 * PLA + 3 * PLD;                                    // one buffer
  static_assert(2 * BUF <= 160 * 1024, "wgrad split LDS");
};

template <int KX>
struct WSGeo {
  static constexpr int KR = KX + FH + 1;          // rows of the output slab (bias row last)
  static constexpr int NI = (KR + 15) / 16;       // i-tiles
  static constexpr int NI0 = (NI + 1) / 2;        // i-tiles of waves 0..3
  static constexpr int JX = (32 * KX / 4 + 511) / 512, JH = (32 * FH / 4 + 511) / 512;  // float4 slots per thread
  static constexpr int JD = (32 * 52 + 511) / 512;  // D slots: 52 float4 per row (the second part uses 48)
  static_assert(KX % 4 == 0 && 16 * NI <= WS_CA, "wgrad split: K");
  using Img = WImg<16 * NI, WS_CD>;
};

// one 16x16x32 operand (8 bf16) of a plane image (row stride ROWB) at column block c0: two
// transposed reads, chunk rows 4 G + q and 16 + 4 G + q of this lane's group G (k = 8 G + j of the
// MFMA maps to chunk row 4 G + j (j < 4) / 16 + 4 G + j - 4: any row order works as long as both
// operands use it; this one keeps a 32-lane read group on 8 consecutive rows); lane_off = the
// lane's (4 G + q) ROWB + 8 p (tr_lane_off)
__device__ __forceinline__ int tr_lane_off(int lane, int rowb) {
  return (4 * (lane >> 4) + ((lane & 15) >> 2)) * rowb + 8 * (lane & 3);
}
template <int ROWB>
__device__ __forceinline__ bf16x8 tr_frag(const lds_char* img, int lane_off, int c0) {
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + lane_off + c0 * 2));
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + lane_off + 16 * ROWB + c0 * 2));
  return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// ------------------------------------------------------------------------------------------
// stages the three split kernels (pair, quad, roles) share; their chunk schedules stay their own
// ------------------------------------------------------------------------------------------
// block -> (row range z, column part jp) with NP column parts per row range; with Z % 8 == 0 the parts of
// a row range sit on one XCD (blocks b, b + 8, ...), so the A rows they all stage come from the same L2
template <int NP>
__device__ __forceinline__ void wg_block(int Z, int& z, int& jp) {
  if (Z % 8 == 0) {
    const unsigned slot = blockIdx.x >> 3;
    jp = slot % NP;
    z = (slot / NP) * 8 + (blockIdx.x & 7);
  } else {
    jp = blockIdx.x % NP;
    z = blockIdx.x / NP;
  }
}
// zero both LDS buffers (pad columns, the zero j-tiles of the last column part)
template <int BYTES>
__device__ __forceinline__ void wg_zero_lds(lds_char* wsm, int tid) {
  for (int i = tid; i < BYTES / 16; i += 512) reinterpret_cast<__attribute__((address_space(3))) u32x4_t*>(wsm)[i] = u32x4_t{0, 0, 0, 0};
}
// bias column (column KR - 1 of the A image) of both buffers, written by threads t < 64: 1 in plane h for
// the primal segment, 0 for the tangent one
template <class GI, int KR>
__device__ __forceinline__ void wg_bias_col(lds_char* wsm, int t, int seg) {
  if (t < 64) {
    const int buf = t >> 5, r = t & 31;
    *reinterpret_cast<__attribute__((address_space(3))) uint16_t*>(wsm + buf * GI::BUF + r * GI::ROWA + (KR - 1) * 2) =
        seg ? 0 : 0x3f80;
  }
}
// Descriptors of one segment's operands for the rows [mb, mb + nr) of a workgroup (a whole-tensor base
// wraps past 4 GiB of dZ: the byte offsets stay 32-bit however large M is).  H starts at row mb - 1 (row
// -1 for mb = 0, whose h_{-1} is never addressed: the t = 0 rows are masked) so every voffset is >= 0 --
// the range check is on voffset alone, and a negative voffset with a compensating soffset reads zeros.
// D starts at the part's first column jbase and ends after its ncol columns of the last row: rows past
// the range read zeros, and so do the columns past 400 of the last row (on the rows before, the kernels
// never address a column >= ncol: wg_slot's nc4).
struct WgRsrc {
  rsrc_t x, h, d;
};
template <int XR>  // XR: X row stride in floats
__device__ __forceinline__ WgRsrc wg_rsrc(const float* X, const float* H, const float* D, int mb, int nr, int jbase, int ncol) {
  return {make_rsrc(X + (size_t)mb * XR, nr * XR * 4), make_rsrc(H + ((ptrdiff_t)mb - 1) * FH, (nr ? nr + 1 : 0) * FH * 4),
          make_rsrc(D + (size_t)mb * FG + jbase, nr ? ((nr - 1) * FG + ncol) * 4 : 0)};
}
// (row mod Tn) of an H staging slot (h_{-1} = 0: the t = 0 rows are not loaded): its value at the first
// chunk, and the advance to the slot's next chunk (step32 = 32 % Tn)
__device__ __forceinline__ int wg_tm0(int mb, int r, int Tn) { return (mb + r) % Tn; }
__device__ __forceinline__ void wg_tm_next(int& tm, int step32, int Tn) {
  tm += step32;
  if (tm >= Tn) tm -= Tn;
}
// element e of the row-major float4 list of a 32-row chunk of one operand, PER float4 per image row (of
// which the first nc4 are real, for a D part narrower than its image): chunk row, float4 column, and
// whether the slot exists
struct WgSlot {
  int r, c4;
  bool ok;
};
template <int PER>
__device__ __forceinline__ WgSlot wg_slot(int e) {
  const int r = e / PER;
  return {r, e - r * PER, e < 32 * PER};
}
template <int PER>
__device__ __forceinline__ WgSlot wg_slot(int e, int nc4) {
  WgSlot s = wg_slot<PER>(e);
  s.ok = s.ok && s.c4 < nc4;
  return s;
}
// a slot's global byte offset in the chunk frame (RS: row stride in floats; kOOB: none) and its LDS byte
// offset in a plane image at byte IMG of the buffer with row stride ROWB (-1: none)
template <int RS>
__device__ __forceinline__ int wg_goff(const WgSlot& s) { return s.ok ? (s.r * RS + 4 * s.c4) * 4 : kOOB; }
template <int ROWB, int IMG>
__device__ __forceinline__ int wg_loff(const WgSlot& s) { return s.ok ? s.r * ROWB + IMG + 8 * s.c4 : -1; }
// per-buffer lane bases of the transposed reads (A image, D image), opaque to the compiler: with the
// buffer and image offsets folded into the reads' immediates they overflowed the 16-bit field
template <class GI>
__device__ __forceinline__ void wg_tr_bases(int lane, int (&tro_a)[2], int (&tro_d)[2]) {
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    tro_a[b] = tr_lane_off(lane, GI::ROWA) + b * GI::BUF;
    tro_d[b] = tr_lane_off(lane, GI::ROWD) + b * GI::BUF + GI::IMGD;
    asm volatile("" : "+v"(tro_a[b]), "+v"(tro_d[b]));
  }
}
// one 16 x 16 accumulator tile (i-tile it, j-tile jt of the part) to the slab:
// C[16 it + 4 g + r][jbase + 16 jt + c16], rows < KR and part columns < ncol
template <int KR>
__device__ __forceinline__ void wg_store_tile(float* out, const f32x4& acc, int it, int jt, int jbase, int ncol, int lane) {
  const int g = lane >> 4, col = 16 * jt + (lane & 15);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = 16 * it + 4 * g + r;
    if (i < KR && col < ncol) out[(size_t)i * FG + jbase + col] = acc[r];
  }
}

// one chunk's products for NIV i-tiles x NJV j-tiles of a wave (acc[ii][jj]): the B planes of the
// NJV j-tiles in registers, the A fragments one i-tile ahead.  Each tile's six products go to a
// fresh accumulator that is added to the running sum in VALU (mma_split6).  Straight-line code (one
// instantiation per wave shape): with a wave-uniform branch between an MFMA and the VALU read of its
// result the compiler did not count the wait states across the branch (2 instead of >= 7).
template <class GI, int NIV, int NJV, int NA, int NB>
__device__ __forceinline__ void ws_chunk(f32x4 (&acc)[NA][NB], const lds_char* A_, const lds_char* D_, int tro_a,
                                         int tro_d, int i0, int j0) {
  bf16x8 bfr[NJV][3];
#pragma unroll
  for (int jj = 0; jj < NJV; ++jj)
#pragma unroll
    for (int q = 0; q < 3; ++q) bfr[jj][q] = tr_frag<GI::ROWD>(D_ + q * GI::PLD, tro_d, 16 * (j0 + jj));
#pragma unroll
  for (int ii = 0; ii < NIV; ++ii) {
    __builtin_amdgcn_sched_barrier(0);
    bf16x8 a3[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) a3[q] = tr_frag<GI::ROWA>(A_ + q * GI::PLA, tro_a, 16 * (i0 + ii));
    // j-tiles in pairs: two fresh accumulators in flight, added after both chains
#pragma unroll
    for (int j2 = 0; j2 < NJV; j2 += 2) {
      f32x4 t[2];
#pragma unroll
      for (int jj = j2; jj < j2 + 2 && jj < NJV; ++jj) t[jj - j2] = mma_split6(a3, bfr[jj], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
      for (int jj = j2; jj < j2 + 2 && jj < NJV; ++jj) acc[ii][jj] += t[jj - j2];
    }
  }
}

// XR: X row stride in floats (35: a 36-column image, column 35 zero).
// Shared with the quad and role kernels: wg_block, wg_zero_lds, wg_bias_col, wg_tm0 / wg_tm_next and, in
// ws_chunk, mma_split6.  The descriptors, the slot tables, the plane stores of `put` and the slab store are
// written out in the parent's form although wg_rsrc, wg_slot / wg_goff / wg_loff, split3_store and
// wg_store_tile compute the same values: through each of them the instruction stream of this kernel, which
// sits at the 256-VGPR cap, moved (through the slot helpers split<32> spilled 38 instead of 35 dwords), and
// with all of them K = 32 with the tangent segment ran 0.03 ms over the parent's 0.02 ms spread
// (profiles/lstmf_grad_split).  As written the four instantiations are instruction-identical to the parent's.
template <int KX, int XR = KX>
__global__ void __launch_bounds__(512, 1)
lstmf_wgrad_split_kernel(const float* __restrict__ X, const float* __restrict__ Hs, const float* __restrict__ D,
                         const float* __restrict__ Xd, const float* __restrict__ Hds, const float* __restrict__ Dd,
                         float* __restrict__ slab, int M, int Tn, int rows_per_z, int Z) {
  constexpr int XRB = 4 * XR, HRB = 4 * FH, DRB = 4 * FG;  // row bytes
  using G = WSGeo<KX>;
  using GI = typename G::Img;
  constexpr int NI = G::NI, NI0 = G::NI0, JX = G::JX, JH = G::JH, JD = G::JD;
  extern __shared__ __attribute__((aligned(16))) char wsm_[];
  lds_char* wsm = (lds_char*)wsm_;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int z, jh;
  wg_block<2>(Z, z, jh);
  const int mb = z * rows_per_z, me = min(M, mb + rows_per_z);
  const int jbase = WS_CD * jh, nd4 = jh ? 48 : 52;  // D columns of this part, float4 per row

  // wave tiles: i-half ig, j-group jg (4 / 3 / 3 / 3 of the 13 local j-tiles)
  const int ig = w >> 2, jg = ig ? 3 - (w & 3) : (w & 3);
  const int i0 = ig ? NI0 : 0, ni = ig ? NI - NI0 : NI0;
  const int j0 = jg == 0 ? 0 : 1 + 3 * jg, nj = jg == 0 ? 4 : 3;

  wg_zero_lds<2 * GI::BUF>(wsm, tid);
  __syncthreads();

  f32x4 acc[NI0][4];
#pragma unroll
  for (int a = 0; a < NI0; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // this lane's transposed-read bases (the D image offset rides in the base VGPR, opaque to the
  // compiler: folded into the reads' immediates it overflowed their 16 bits and cost a register per read)
  const int tro_a = tr_lane_off(lane, GI::ROWA);
  int tro_d = tr_lane_off(lane, GI::ROWD) + GI::IMGD;
  asm volatile("" : "+v"(tro_d));

  // per-thread float4 slots of a 32-row chunk: X (JX), H (JH), D (JD); element e = tid + 512 j:
  // byte offset in the chunk frame (kOOB: none), LDS byte offset (-1: none), H-slot row
  int gx[JX], lx[JX], gh[JH], lh[JH], rhr[JH], gd[JD], ld_[JD], rd_[JD];
#pragma unroll
  for (int j = 0; j < JX; ++j) {
    const int e = tid + 512 * j, r = e / (KX / 4), c4 = e - r * (KX / 4);
    const bool ok = e < 32 * KX / 4;
    gx[j] = ok ? (r * XR + 4 * c4) * 4 : kOOB;
    lx[j] = ok ? r * GI::ROWA + 8 * c4 : -1;
  }
#pragma unroll
  for (int j = 0; j < JH; ++j) {
    const int e = tid + 512 * j, r = e / (FH / 4), c4 = e - r * (FH / 4);
    const bool ok = e < 32 * FH / 4;
    gh[j] = ok ? (r * FH + 4 * c4) * 4 : kOOB;
    lh[j] = ok ? r * GI::ROWA + 2 * KX + 8 * c4 : -1;
    rhr[j] = ok ? r : 0;
  }
#pragma unroll
  for (int j = 0; j < JD; ++j) {
    const int e = tid + 512 * j, r = e / 52, c4 = e - r * 52;
    const bool ok = e < 32 * 52 && c4 < nd4;
    gd[j] = ok ? (r * FG + jbase + 4 * c4) * 4 : kOOB;
    ld_[j] = ok ? GI::IMGD + r * GI::ROWD + 8 * c4 : -1;
    rd_[j] = ok ? r : 0;
  }
  const int step32 = 32 % Tn;

  f32x4 vx[JX], vh[JH], vd[JD];
  for (int seg = 0; seg < (Xd ? 2 : 1); ++seg) {
    const char* Xs = reinterpret_cast<const char*>(seg ? Xd : X);
    const char* Hq = reinterpret_cast<const char*>(seg ? Hds : Hs);
    const char* Dq = reinterpret_cast<const char*>(seg ? Dd : D);
    // the H descriptor starts at row mb - 1 (row -1 for mb = 0, whose h_{-1} is never addressed: the
    // t = 0 rows are masked) so every voffset is >= 0 -- the range check is on voffset alone, and a
    // negative voffset with a compensating soffset reads zeros
    const int nr = me > mb ? me - mb : 0;
    const rsrc_t rx = make_rsrc(Xs + (size_t)mb * XRB, nr * XRB);
    const rsrc_t rh = make_rsrc(Hq + ((ptrdiff_t)mb - 1) * HRB, (nr ? nr + 1 : 0) * HRB);
    const rsrc_t rd = make_rsrc(Dq + (size_t)mb * DRB, nr * DRB);
    // t = (row) mod Tn of this thread's H slots at the current chunk (h_{-1} = 0 rows)
    int tm[JH];
#pragma unroll
    for (int j = 0; j < JH; ++j) tm[j] = wg_tm0(mb, rhr[j], Tn);
    auto load = [&](int m0) {  // rows past me: voffset out of range, zeros
      const int lim = me - m0;
#pragma unroll
      for (int j = 0; j < JX; ++j) {
        vx[j] = ldx4<XR>(rx, (gx[j] >> 2) / XR < lim ? gx[j] : kOOB, (m0 - mb) * XRB, (gx[j] >> 2) % XR);
      }
#pragma unroll
      for (int j = 0; j < JH; ++j) {
        const int vo = rhr[j] < lim && tm[j] != 0 ? gh[j] : kOOB;
        vh[j] = ld4s(rh, vo, (m0 - mb) * HRB);
      }
#pragma unroll
      for (int j = 0; j < JD; ++j) {
        const int vo = rd_[j] < lim ? gd[j] : kOOB;
        vd[j] = ld4s(rd, vo, (m0 - mb) * DRB);
      }
#pragma unroll
      for (int j = 0; j < JH; ++j) {
        wg_tm_next(tm[j], step32, Tn);
      }
    };
    auto put = [&](lds_char* base, int lo, const f32x4& v) {
      if (lo >= 0) {
        uint32_t p[3][2];
        split3(v, p);
        const int pl = lo < GI::IMGD ? GI::PLA : GI::PLD;
#pragma unroll
        for (int q = 0; q < 3; ++q)
          *reinterpret_cast<__attribute__((address_space(3))) u32x2_t*>(base + lo + q * pl) = u32x2_t{p[q][0], p[q][1]};
      }
    };
    auto stage = [&](int buf) {
      lds_char* base = wsm + buf * GI::BUF;
#pragma unroll
      for (int j = 0; j < JX; ++j) put(base, lx[j], vx[j]);
#pragma unroll
      for (int j = 0; j < JH; ++j) put(base, lh[j], vh[j]);
#pragma unroll
      for (int j = 0; j < JD; ++j) put(base, ld_[j], vd[j]);
    };
    // bias column (column KR - 1 of A): 1 in plane h for the primal segment, 0 for the tangent one
    wg_bias_col<GI, G::KR>(wsm, tid, seg);
    const int nch = nr > 0 ? (nr + 31) / 32 : 0;
    if (nch > 0) {
      load(mb);
      stage(0);
    }
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
      const bool more = c + 1 < nch;
      if (more) load(mb + 32 * (c + 1));
      const lds_char* A_ = wsm + (c & 1) * GI::BUF;
      const lds_char* D_ = A_;  // (+ IMGD in tro_d)
      switch (ni * 8 + nj) {
        case NI0 * 8 + 4: ws_chunk<GI, NI0, 4>(acc, A_, D_, tro_a, tro_d, i0, j0); break;
        case NI0 * 8 + 3: ws_chunk<GI, NI0, 3>(acc, A_, D_, tro_a, tro_d, i0, j0); break;
        case (NI - NI0) * 8 + 4: ws_chunk<GI, NI - NI0, 4>(acc, A_, D_, tro_a, tro_d, i0, j0); break;
        default: ws_chunk<GI, NI - NI0, 3>(acc, A_, D_, tro_a, tro_d, i0, j0); break;
      }
      if (more) stage((c + 1) & 1);
      __syncthreads();
    }
    __syncthreads();  // (the bias column of both buffers is rewritten for the next segment)
  }
  // slab store: C[16 (i0 + ii) + 4 g + r][jbase + 16 (j0 + jj) + c16]
  float* out = slab + (size_t)z * G::KR * FG;
  const int g = lane >> 4, c16 = lane & 15;
#pragma unroll
  for (int ii = 0; ii < NI0; ++ii)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
      if (ii < ni && jj < nj) {
        const int col = jbase + 16 * (j0 + jj) + c16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * (i0 + ii) + 4 * g + r;
          if (i < G::KR && col < FG) out[(size_t)i * FG + col] = acc[ii][jj][r];
        }
      }
}

// ------------------------------------------------------------------------------------------
// split weight gradient, column QUAD: lstmf_wgrad_q4_kernel
// ------------------------------------------------------------------------------------------
// lstmf_wgrad_split_kernel (a workgroup PAIR per row range, 208 columns each) runs its 8 waves in one
// phase at a time -- load -> MFMAs -> split + LDS store -> barrier -- so the matrix pipe idles through
// the split (39.5 % MFMA busy at K = 32), and at K = 100 its 28-tile waves spill (53 ms vs 16 ms
// exact).  Here FOUR workgroups share a row range and split the 400 gate columns in quarters of 100
// (7 j-tiles, the last one 4 / 16 real); the quad sits on one XCD (blocks b, b + 8, b + 16, b + 24),
// so the A rows [x | h_{t-1} | 1] that all four stage come from the same L2.  8 waves (2 per SIMD):
// the NI x 7 output tiles are dealt out as i-groups x j-groups (<= 4 x 4 per wave), so a wave keeps
// its accumulators and <= 2 j-tiles' D fragments in registers and streams the A fragments.
// Prefetch distance two chunks: chunk c + 2's fp32 rows are loaded at the top of chunk c (two
// register sets alternate), and chunk c + 1's rows are split and stored into the other LDS buffer in
// slices between chunk c's i-tiles, so the HBM latency hides under 1.5 chunks of MFMAs and the
// split's VALU issue interleaves with the MFMAs of the same and the partner wave.  Same products and
// accumulation as lstmf_wgrad_split_kernel: six bf16 products per tile into a fresh accumulator,
// added to the running sum in VALU fp32.
constexpr int WQ_CD = 100, WQ_NJ = 7, WQ_W = 8;  // D columns per part, j-tiles per part, waves
template <int KX>
struct WQGeo {
  static constexpr int KR = KX + FH + 1;
  static constexpr int NI = (KR + 15) / 16;
  static constexpr int NIG = (NI + 3) / 4;                  // i-tiles of the first i-group (the rest NI / 4)
  static constexpr int MAXT = NIG * 4;                      // tiles per wave (max): <= 4 i x 4 j
  static constexpr int JX = (32 * KX / 4 + 511) / 512, JH = (32 * FH / 4 + 511) / 512;
  static constexpr int JD = (32 * WQ_CD / 4 + 511) / 512;
  static constexpr int NS = JX + JH + JD;                   // float4 staging slots per thread
  static_assert(KX % 4 == 0 && 16 * NI <= WS_CA && NI <= 16, "wgrad q4: K");
  // wave w: i-group ig, j-group jg (j-tiles 0-3 / 4-6); the two waves of a SIMD (w, w + 4) take
  // mirrored i-groups so the SIMDs carry 25 / 21 / 21 / 24 tiles at K = 100
  static constexpr int ig(int w) { return w < 4 ? w : 3 - (w & 3); }
  static constexpr int i0(int g) { return g == 0 ? 0 : NIG + (g - 1) * ((NI - NIG) / 3) + ((g - 1) < (NI - NIG) % 3 ? g - 1 : (NI - NIG) % 3); }
  static constexpr int ni(int g) { return i0(g + 1 > 3 ? 3 : g + 1) - i0(g) + (g == 3 ? NI - i0(3) : 0); }
  static constexpr int j0(int w) { return w < 4 ? 0 : 4; }
  static constexpr int nj(int w) { return w < 4 ? 4 : 3; }
  using Img = WImg<16 * NI, 16 * WQ_NJ>;
};

// Shared with the pair and role kernels: wg_block, wg_zero_lds, wg_bias_col, wg_slot (the coordinates are
// recomputed at every use instead of held in tables: registers), wg_tm0 and mma_split6.  The transposed-read
// bases, the descriptors, the (row mod Tn) advance, the offsets and plane stores of `stage` and the slab store
// are written out in the parent's form although wg_tr_bases, wg_rsrc, wg_tm_next, wg_goff / wg_loff,
// split3_store and wg_store_tile compute the same values: each of them moved this kernel's instruction
// stream, through wg_loff + split3_store K = 32 / 36 took 222 / 220 VGPRs instead of 220 / 218, and with all of
// them K = 100 ran 0.6 - 0.7 % slower than the parent's (13.98 -> 14.06 ms, profiles/lstmf_grad_split).
template <int KX>
__global__ void __launch_bounds__(512, 1)
lstmf_wgrad_q4_kernel(const float* __restrict__ X, const float* __restrict__ Hs, const float* __restrict__ D,
                      const float* __restrict__ Xd, const float* __restrict__ Hds, const float* __restrict__ Dd,
                      float* __restrict__ slab, int M, int Tn, int rows_per_z, int Z) {
  constexpr int XRB = 4 * KX, HRB = 4 * FH, DRB = 4 * FG;  // row bytes
  using G = WQGeo<KX>;
  using GI = typename G::Img;
  constexpr int JX = G::JX, JH = G::JH, NS = G::NS, MAXT = G::MAXT;
  extern __shared__ __attribute__((aligned(16))) char wsm_[];
  lds_char* wsm = (lds_char*)wsm_;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int z, jq;
  wg_block<4>(Z, z, jq);
  const int mb = z * rows_per_z, me = min(M, mb + rows_per_z);
  const int jbase = WQ_CD * jq;

  wg_zero_lds<2 * GI::BUF>(wsm, tid);
  __syncthreads();

  f32x4 acc[MAXT];
#pragma unroll
  for (int a = 0; a < MAXT; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};

  // per-buffer lane bases of the transposed reads (A image, D image), opaque to the compiler: with the
  // buffer and image offsets folded into the reads' immediates they overflowed the 16-bit field
  int tro_a[2], tro_d[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    tro_a[b] = tr_lane_off(lane, GI::ROWA) + b * GI::BUF;
    tro_d[b] = tr_lane_off(lane, GI::ROWD) + b * GI::BUF + GI::IMGD;
    asm volatile("" : "+v"(tro_a[b]), "+v"(tro_d[b]));
  }
  const int step32 = 32 % Tn;

  // staging slot s of this thread: kind (x / h / d) is compile-time in s
  auto slot_rc = [&](int s, int& r, int& c4, bool& ok) {
    WgSlot sl;
    if (s < JX) sl = wg_slot<KX / 4>(tid + 512 * s);
    else if (s < JX + JH) sl = wg_slot<FH / 4>(tid + 512 * (s - JX));
    else sl = wg_slot<WQ_CD / 4>(tid + 512 * (s - JX - JH));
    r = sl.r; c4 = sl.c4; ok = sl.ok;
    if (!ok) r = c4 = 0;
  };

  f32x4 v[NS];
  for (int seg = 0; seg < (Xd ? 2 : 1); ++seg) {
    const char* Xs = reinterpret_cast<const char*>(seg ? Xd : X);
    const char* Hq = reinterpret_cast<const char*>(seg ? Hds : Hs);
    const char* Dq = reinterpret_cast<const char*>(seg ? Dd : D);
    const int nr = me > mb ? me - mb : 0;
    const rsrc_t rx = make_rsrc(Xs + (size_t)mb * XRB, nr * XRB);
    // (row mb - 1 based: every voffset >= 0; h_{-1} rows are masked by t)
    const rsrc_t rh = make_rsrc(Hq + ((ptrdiff_t)mb - 1) * HRB, (nr ? nr + 1 : 0) * HRB);
    const rsrc_t rd = make_rsrc(Dq + (size_t)mb * DRB + jbase * 4, nr ? (nr - 1) * DRB + WQ_CD * 4 : 0);
    int tm[JH];  // (row mod Tn) of this thread's H slots at the next chunk to load
#pragma unroll
    for (int j = 0; j < JH; ++j) {
      int r, c4;
      bool ok;
      slot_rc(JX + j, r, c4, ok);
      tm[j] = wg_tm0(mb, r, Tn);
    }
    // slot s of the chunk at row m0 into the register set (rows past me -- or past the range -- read
    // zeros); an H slot's (row mod Tn) then advances to its next chunk
    auto load_slot = [&](int s, int m0) {
      int r, c4;
      bool ok;
      slot_rc(s, r, c4, ok);
      ok = ok && r < me - m0;
      if (s < JX) {
        v[s] = ld4s(rx, ok ? (r * KX + 4 * c4) * 4 : kOOB, (m0 - mb) * XRB);
      } else if (s < JX + JH) {
        int& tmj = tm[s - JX];
        v[s] = ld4s(rh, ok && tmj != 0 ? (r * FH + 4 * c4) * 4 : kOOB, (m0 - mb) * HRB);
        tmj += step32;
        if (tmj >= Tn) tmj -= Tn;
      } else {
        v[s] = ld4s(rd, ok ? (r * FG + 4 * c4) * 4 : kOOB, (m0 - mb) * DRB);
      }
    };
    auto stage = [&](lds_char* base, int s) {
      int r, c4;
      bool ok;
      slot_rc(s, r, c4, ok);
      if (!ok) return;
      int lo, pl;
      if (s < JX) { lo = r * GI::ROWA + 8 * c4; pl = GI::PLA; }
      else if (s < JX + JH) { lo = r * GI::ROWA + 2 * KX + 8 * c4; pl = GI::PLA; }
      else { lo = GI::IMGD + r * GI::ROWD + 8 * c4; pl = GI::PLD; }
      uint32_t p[3][2];
      split3(v[s], p);
#pragma unroll
      for (int q = 0; q < 3; ++q)
        *reinterpret_cast<__attribute__((address_space(3))) u32x2_t*>(base + lo + q * pl) = u32x2_t{p[q][0], p[q][1]};
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    wg_bias_col<GI, G::KR>(wsm, tid, seg);
    const int nch = nr > 0 ? (nr + 31) / 32 : 0;
    // prologue: chunk 0 staged into buffer 0, chunk 1 in flight in the register set
#pragma unroll
    for (int s = 0; s < NS; ++s) load_slot(s, mb);
#pragma unroll
    for (int s = 0; s < NS; ++s) stage(wsm, s);
#pragma unroll
    for (int s = 0; s < NS; ++s) load_slot(s, mb + 32);
    __syncthreads();
    // chunk c (S = c & 1): MFMAs on buffer S; between the i-tiles the set's slots (chunk c + 1) are
    // split into buffer S ^ 1, each slot reloaded with chunk c + 2 right after (one register set:
    // a slot's HBM latency hides under one chunk of MFMAs)
    auto chunk = [&](auto S_, int c) {
      constexpr int S = decltype(S_)::value;
      const lds_char* A_ = wsm;  // (+ S BUF in tro_a[S], + S BUF + IMGD in tro_d[S])
      const lds_char* D_ = wsm;
      lds_char* nxt = wsm + (S ^ 1) * GI::BUF;
      // one straight-line body per wave (no branch between an MFMA and the VALU read of its
      // result); wave W owns tiles [TS, TE) of the j-major list (tile L = j NI + i).  The staging
      // slices are unconditional: after the last chunk they store the (zero) rows past the range
      // into the idle buffer
      auto body = [&](auto WK) {
        constexpr int W = decltype(WK)::value;
        constexpr int IG = G::ig(W), I0 = G::i0(IG), NIW = G::ni(IG), J0 = G::j0(W), NJW = G::nj(W);
        constexpr int NJH = (NJW + 1) / 2;                  // j-tiles in pairs: 2 x 3 D fragments held
        constexpr int SPI = (NS + NJH * NIW - 1) / (NJH * NIW);  // staging slots per (pair, i-tile)
        auto jpair = [&](auto JH_) {  // (a lambda per pair: the slot indices below stay compile-time)
          constexpr int jh = decltype(JH_)::value;
          bf16x8 bfr[2][3];
#pragma unroll
          for (int jj = 0; jj < 2; ++jj)
            if (2 * jh + jj < NJW) {
#pragma unroll
              for (int q = 0; q < 3; ++q) bfr[jj][q] = tr_frag<GI::ROWD>(D_ + q * GI::PLD, tro_d[S], 16 * (J0 + 2 * jh + jj));
            }
          // A fragments one i-tile ahead (two sets) where the registers allow (K <= 36): the LDS
          // latency hides under the MFMAs
          constexpr bool PF = KX <= 36;
          bf16x8 af[2][3];
#pragma unroll
          for (int q = 0; q < 3; ++q) af[0][q] = tr_frag<GI::ROWA>(A_ + q * GI::PLA, tro_a[S], 16 * I0);
#pragma unroll
          for (int ii = 0; ii < NIW; ++ii) {
            __builtin_amdgcn_sched_barrier(0);
            if (PF && ii + 1 < NIW) {
#pragma unroll
              for (int q = 0; q < 3; ++q) af[(ii + 1) & 1][q] = tr_frag<GI::ROWA>(A_ + q * GI::PLA, tro_a[S], 16 * (I0 + ii + 1));
            } else if (!PF && ii > 0) {
#pragma unroll
              for (int q = 0; q < 3; ++q) af[ii & 1][q] = tr_frag<GI::ROWA>(A_ + q * GI::PLA, tro_a[S], 16 * (I0 + ii));
            }
            const bf16x8(&a3)[3] = af[ii & 1];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
              if (2 * jh + jj >= NJW) continue;  // (compile-time)
              acc[ii * 4 + 2 * jh + jj] += mma_split6(a3, bfr[jj], f32x4{0.f, 0.f, 0.f, 0.f});
            }
            const int it = jh * NIW + ii;
#pragma unroll
            for (int s = it * SPI; s < (it + 1) * SPI && s < NS; ++s) {
              stage(nxt, s);
              load_slot(s, mb + 32 * (c + 2));
            }
          }
        };
        jpair(std::integral_constant<int, 0>{});
        if constexpr (NJH > 1) jpair(std::integral_constant<int, 1>{});
      };
      switch (w) {
        case 0: body(std::integral_constant<int, 0>{}); break;
        case 1: body(std::integral_constant<int, 1>{}); break;
        case 2: body(std::integral_constant<int, 2>{}); break;
        case 3: body(std::integral_constant<int, 3>{}); break;
        case 4: body(std::integral_constant<int, 4>{}); break;
        case 5: body(std::integral_constant<int, 5>{}); break;
        case 6: body(std::integral_constant<int, 6>{}); break;
        default: body(std::integral_constant<int, 7>{}); break;
      }
      __syncthreads();
    };
    int c = 0;
    for (; c + 1 < nch; c += 2) {
      chunk(I0{}, c);
      chunk(I1{}, c + 1);
    }
    if (c < nch) chunk(I0{}, c);
    __syncthreads();  // (the bias column of both buffers is rewritten for the next segment)
  }
  // slab store: acc[4 ii + jj] -> C[16 (i0 + ii) + 4 g + r][jbase + 16 (j0 + jj) + c16]
  float* out = slab + (size_t)z * G::KR * FG;
  const int g = lane >> 4, c16 = lane & 15;
  const int igw = G::ig(w), i0w = G::i0(igw), niw = G::ni(igw), j0w = G::j0(w), njw = G::nj(w);
#pragma unroll
  for (int ii = 0; ii < G::NIG; ++ii)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int col = 16 * (j0w + jj) + c16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * (i0w + ii) + 4 * g + r;
        if (ii < niw && jj < njw && i < G::KR && col < WQ_CD)
          out[(size_t)i * FG + jbase + col] = acc[ii * 4 + jj][r];
      }
    }
}

// ------------------------------------------------------------------------------------------
// split weight gradient, MFMA and staging ROLES: lstmf_wgrad_roles_kernel
// ------------------------------------------------------------------------------------------
// lstmf_wgrad_split_kernel and lstmf_wgrad_q4_kernel run eight identical waves: each reads its A
// fragments from LDS, issues the MFMA chains, adds the fresh accumulators in VALU and runs its slice
// of the next chunk's staging (global loads, split3, LDS stores).  A wave issues in order and there
// are two per SIMD, so LDS latency, MFMA result latency and the staging VALU alternate instead of
// overlapping (31 - 38 % MFMA busy, about twice the kernels' own issue bound), and both kernels sit at
// the 256-register cap with spills.  Here the two jobs go to different waves that share a SIMD, as in
// lstmf_bwdp_kernel: waves 0-3 are MFMA waves, waves 4-7 staging waves (the waves of a workgroup go
// round the SIMDs, so every SIMD hosts one of each).
//   staging waves: every global access.  Chunk c + 2's fp32 rows are loaded at the top of chunk c (two
//     register sets alternate), then chunk c + 1's rows are split and stored into LDS buffer S ^ 1.
//   MFMA waves: no global memory instruction, their only waits are on LDS.  Wave w owns the tiles
//     [ts(w), ts(w + 1)) of the j-major list L = j NI + i (23 / 23 / 23 / 22 of 13 x 7 at K = 100,
//     30 / 29 / 29 / 29 of 9 x 13 at K = 32), keeps the D fragments of its <= 4 j-tiles for the chunk
//     and walks its tiles i-major with the A fragments one i-tile ahead: every operand is read from LDS
//     once per wave.  Two fresh accumulators alternate, and tile n's VALU add is issued after tile
//     n + 1's MFMAs, so no MFMA result wait is exposed.
// One workgroup barrier per chunk separates "buffer S consumed" from "buffer S ^ 1 produced".  The role
// branch is taken once, outside the chunk loop; each role's chunk body is straight-line code.
// Arithmetic, workgroup partition (column pair of 208 for K <= 36, column quad of 100 above), row
// ranges, slab and LDS images are those of the pair / quad kernel: a tile's six products go in the same
// order into a zeroed accumulator that is added to the running sum once per chunk, so the result is
// bitwise that of lstmf_wgrad_split_kernel (K = 32) / lstmf_wgrad_q4_kernel (K = 100).
#ifndef HFREP_WGRAD_ROLES_APF
#define HFREP_WGRAD_ROLES_APF 1  // i-tiles of lead of the MFMA waves' A-fragment reads (A/B: docs/PERF.md)
#endif
#ifndef HFREP_WGRAD_ROLES_PRIO
#define HFREP_WGRAD_ROLES_PRIO 0  // 1: the MFMA waves at priority 1 for the chunk loop (A/B: docs/PERF.md)
#endif
template <int KX>
struct WRGeo {
  static constexpr bool QUAD = KX > 36;
  static constexpr int NP = QUAD ? 4 : 2;                   // column parts per row range
  static constexpr int CDP = QUAD ? WQ_CD : WS_CD;          // D columns per part
  static constexpr int NJ = (CDP + 15) / 16;                // j-tiles per part
  static constexpr int KR = KX + FH + 1;
  static constexpr int NI = (KR + 15) / 16;
  static constexpr int NT = NI * NJ;                        // output tiles per workgroup
  static constexpr int ts(int w) { return w * (NT / 4) + (w < NT % 4 ? w : NT % 4); }  // first tile of MFMA wave w
  static constexpr int MAXT = (NT + 3) / 4;
  static constexpr int ND4 = CDP / 4;                       // float4 per D image row
  static constexpr int JX = (32 * KX / 4 + 255) / 256, JH = (32 * FH / 4 + 255) / 256, JD = (32 * ND4 + 255) / 256;
  static constexpr int NS = JX + JH + JD;                   // float4 staging slots per staging lane
  static_assert(KX % 4 == 0 && CDP % 4 == 0 && 16 * NI <= WS_CA && MAXT * 4 <= 120, "wgrad roles: K");
  using Img = WImg<16 * NI, 16 * NJ>;
};

template <int KX>
__global__ void __launch_bounds__(512, 1)
lstmf_wgrad_roles_kernel(const float* __restrict__ X, const float* __restrict__ Hs, const float* __restrict__ D,
                         const float* __restrict__ Xd, const float* __restrict__ Hds, const float* __restrict__ Dd,
                         float* __restrict__ slab, int M, int Tn, int rows_per_z, int Z) {
  using G = WRGeo<KX>;
  using GI = typename G::Img;
  constexpr int NI = G::NI, NP = G::NP, JX = G::JX, JH = G::JH, NS = G::NS;
  constexpr int XRB = 4 * KX, HRB = 4 * FH, DRB = 4 * FG;  // row bytes
  extern __shared__ __attribute__((aligned(16))) char wsm_[];
  lds_char* wsm = (lds_char*)wsm_;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int z, jp;
  wg_block<NP>(Z, z, jp);
  const int mb = z * rows_per_z, me = min(M, mb + rows_per_z);
  const int jbase = G::CDP * jp, ncol = min(G::CDP, FG - jbase);  // real D columns of this part
  const int nr = me > mb ? me - mb : 0, nch = (nr + 31) / 32;
  const int nseg = Xd ? 2 : 1;

  wg_zero_lds<2 * GI::BUF>(wsm, tid);
  __syncthreads();

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  // barriers per segment, both roles: one after the prologue (buffer 0 and the bias column staged), one
  // per chunk
  if (w < 4) {
    // ---------------- MFMA role ----------------
    auto role = [&](auto WK) {
      constexpr int W = decltype(WK)::value;
      constexpr int TS = G::ts(W), TE = G::ts(W + 1), JA = TS / NI, NJW = (TE - 1) / NI - JA + 1;
      f32x4 acc[TE - TS];
#pragma unroll
      for (int a = 0; a < TE - TS; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
      int tro_a[2], tro_d[2];
      wg_tr_bases<GI>(lane, tro_a, tro_d);
      auto chunk = [&](auto S_) {
        constexpr int S = decltype(S_)::value;
        bf16x8 bfr[NJW][3];
#pragma unroll
        for (int jj = 0; jj < NJW; ++jj)
#pragma unroll
          for (int q = 0; q < 3; ++q) bfr[jj][q] = tr_frag<GI::ROWD>(wsm + q * GI::PLD, tro_d[S], 16 * (JA + jj));
        constexpr int PF = HFREP_WGRAD_ROLES_APF;  // A fragments PF i-tiles ahead, PF + 1 sets
        bf16x8 af[PF + 1][3];
#pragma unroll
        for (int i = 0; i < PF; ++i)
#pragma unroll
          for (int q = 0; q < 3; ++q) af[i][q] = tr_frag<GI::ROWA>(wsm + q * GI::PLA, tro_a[S], 16 * i);
        f32x4 t[2];
        int pend = -1, par = 0;  // (compile-time after unrolling) tile whose add is outstanding, fresh set
#pragma unroll
        for (int ii = 0; ii < NI; ++ii) {
          __builtin_amdgcn_sched_barrier(0);
          if (ii + PF < NI) {
#pragma unroll
            for (int q = 0; q < 3; ++q) af[(ii + PF) % (PF + 1)][q] = tr_frag<GI::ROWA>(wsm + q * GI::PLA, tro_a[S], 16 * (ii + PF));
          }
          __builtin_amdgcn_sched_barrier(0);  // (the prefetch ahead of this i-tile's MFMAs: a full i-tile of lead)
          const bf16x8(&a3)[3] = af[ii % (PF + 1)];
#pragma unroll
          for (int jj = 0; jj < NJW; ++jj) {
            const int L = (JA + jj) * NI + ii;
            if (L < TS || L >= TE) continue;  // (compile-time)
            t[par] = mma_split6(a3, bfr[jj], f32x4{0.f, 0.f, 0.f, 0.f});
            __builtin_amdgcn_sched_barrier(0);
            if (pend >= 0) acc[pend] += t[par ^ 1];  // the previous tile's add, behind this tile's MFMAs
            pend = L - TS;
            par ^= 1;
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        acc[pend] += t[par ^ 1];
      };
#if HFREP_WGRAD_ROLES_PRIO
      __builtin_amdgcn_s_setprio(1);
#endif
      for (int seg = 0; seg < nseg; ++seg) {
        lds_barrier();
        int c = 0;
        for (; c + 1 < nch; c += 2) {
          chunk(I0{});
          lds_barrier();
          chunk(I1{});
          lds_barrier();
        }
        if (c < nch) {
          chunk(I0{});
          lds_barrier();
        }
      }
      // slab store: tile L = TS + n -> C[16 i + 4 g + r][jbase + 16 j + c16]
      float* out = slab + (size_t)z * G::KR * FG;
#pragma unroll
      for (int n = 0; n < TE - TS; ++n) wg_store_tile<G::KR>(out, acc[n], (TS + n) % NI, (TS + n) / NI, jbase, ncol, lane);
    };
    switch (w) {
      case 0: role(std::integral_constant<int, 0>{}); break;
      case 1: role(std::integral_constant<int, 1>{}); break;
      case 2: role(std::integral_constant<int, 2>{}); break;
      default: role(std::integral_constant<int, 3>{}); break;
    }
  } else {
    // ---------------- staging role ----------------
    const int st = tid - 256;
    // float4 slot s of this lane in a 32-row chunk: X (JX slots), H (JH), D (JD); element e = lane' +
    // 256 j of the kind's row-major list, the lane index rotated by a wave per kind so the ragged last
    // slots of the three kinds fall on different waves.  gv: byte offset in the chunk frame (kOOB:
    // none), lo: LDS byte offset (-1: none), rr: chunk row
    int gv[NS], lo[NS], rr[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      WgSlot sl;
      if (s < JX) {
        sl = wg_slot<KX / 4>(st + 256 * s);
        gv[s] = wg_goff<KX>(sl);
        lo[s] = wg_loff<GI::ROWA, 0>(sl);
      } else if (s < JX + JH) {
        sl = wg_slot<FH / 4>(((st + 64) & 255) + 256 * (s - JX));
        gv[s] = wg_goff<FH>(sl);
        lo[s] = wg_loff<GI::ROWA, 2 * KX>(sl);
      } else {
        sl = wg_slot<G::ND4>(((st + 128) & 255) + 256 * (s - JX - JH), ncol / 4);
        gv[s] = wg_goff<FG>(sl);
        lo[s] = wg_loff<GI::ROWD, GI::IMGD>(sl);
      }
      rr[s] = sl.ok ? sl.r : 0;
    }
    const int step32 = 32 % Tn;
    f32x4 v[2][NS];
    for (int seg = 0; seg < nseg; ++seg) {
      const WgRsrc rs = wg_rsrc<KX>(seg ? Xd : X, seg ? Hds : Hs, seg ? Dd : D, mb, nr, jbase, ncol);
      int tm[JH];  // (row mod Tn) of this lane's H slots at the next chunk to load
#pragma unroll
      for (int j = 0; j < JH; ++j) tm[j] = wg_tm0(mb, rr[JX + j], Tn);
      // the chunk at row m0 into register set Q (rows past me read zeros: voffset out of range); an H
      // slot's (row mod Tn) then advances to its next chunk
      auto load = [&](auto Q_, int m0) {
        constexpr int Q = decltype(Q_)::value;
        const int lim = me - m0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const bool in = rr[s] < lim;
          if (s < JX) {
            v[Q][s] = ld4s(rs.x, in ? gv[s] : kOOB, (m0 - mb) * XRB);
          } else if (s < JX + JH) {
            int& tmj = tm[s - JX];
            v[Q][s] = ld4s(rs.h, in && tmj != 0 ? gv[s] : kOOB, (m0 - mb) * HRB);
            wg_tm_next(tmj, step32, Tn);
          } else {
            v[Q][s] = ld4s(rs.d, in ? gv[s] : kOOB, (m0 - mb) * DRB);
          }
        }
      };
      // register set Q split into the three planes of buffer `buf`
      auto stage = [&](auto Q_, int buf) {
        constexpr int Q = decltype(Q_)::value;
        lds_char* base = wsm + buf * GI::BUF;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          if (lo[s] >= 0) split3_store(v[Q][s], base + lo[s], s < JX + JH ? GI::PLA : GI::PLD);
        }
      };
      // bias column KR - 1 of A: 1 in plane h for the primal segment, 0 for the tangent one.  (Every
      // MFMA wave is past the last chunk's barrier of the previous segment: both buffers are idle.)
      wg_bias_col<GI, G::KR>(wsm, st, seg);
      // prologue: chunk 0 staged into buffer 0, chunk 1 in flight in set 1
      load(I0{}, mb);
      stage(I0{}, 0);
      load(I1{}, mb + 32);
      lds_barrier();
      // chunk c (S = c & 1): chunk c + 2's loads into set S (its rows went to buffer S during chunk
      // c - 1), then set S ^ 1 (chunk c + 1) into buffer S ^ 1.  Unconditional: after the last chunk the
      // (zero) rows past the range go to the idle buffer
      int c = 0;
      for (; c + 1 < nch; c += 2) {
        load(I0{}, mb + 32 * (c + 2));
        stage(I1{}, 1);
        lds_barrier();
        load(I1{}, mb + 32 * (c + 3));
        stage(I0{}, 0);
        lds_barrier();
      }
      if (c < nch) {
        load(I0{}, mb + 32 * (c + 2));
        stage(I1{}, 1);
        lds_barrier();
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// fp32 input gradient on the bf16 matrix pipe, LDS-staged: lstmf_dgrad_s4_kernel
// ------------------------------------------------------------------------------------------
// dX = dZ W^T with the exact three-term split (six products, dropped terms <= 2^-24 of each product).
// An earlier split kernel spread the 400-long reduction over its 8 waves and reduced their partial
// tiles in LDS per 16-row tile (barrier + 8-way sum per tile: slower than the exact kernel).  Here the
// reduction stays inside one wave: 4 waves (one per SIMD, 512-register budget), wave w owns output
// columns 32 w .. 32 w + 31 (two 16-column tiles) and holds the three W^T planes of BOTH tiles and ALL 13
// k-steps (k = 400..415 zero) in registers (312 VGPRs).  The 16-row dZ chunks are fp32-loaded two chunks
// ahead (two register sets), split into the three bf16 planes and stored to a double-buffered LDS image
// (row stride 424 elements: conflict-free ds_read_b128 A fragments) in slices between the second half
// of the k-steps, so the split's VALU issue interleaves with the wave's MFMAs.  One barrier per chunk;
// each chunk's output tiles are final (no partial tiles, no cross-wave reduction).
constexpr int DS4_RS = 432;                   // LDS image row stride (bf16 elements): >= 416, conflict-free b128
constexpr int DS4_PL = 16 * DS4_RS * 2;       // bytes per plane image (16 rows)
constexpr int DS4_BUF = 3 * DS4_PL;           // one buffer: three planes
constexpr int DS4_SLOTS = (16 * 100 + 255) / 256;  // float4 staging slots per thread per chunk (7)
constexpr int DS4_K0 = DS_KS - DS4_SLOTS;     // first k-step followed by a staging slot
// register sets of the dZ prefetch: 2 = one chunk ahead (three sets, two chunks ahead, measured
// 3.59 vs 3.54 ms at 6.3 M rows: profiles/r04_wgrad/wdma2)
constexpr int DS4_NS = 2;

template <int NT2>
__global__ void __launch_bounds__(256, 1)
lstmf_dgrad_s4_kernel(const float* __restrict__ D, const float* __restrict__ W, float* __restrict__ X, int M, int KO) {
  constexpr int DRB = 4 * FG;  // dZ row bytes
  extern __shared__ __attribute__((aligned(16))) char dsm_[];
  lds_char* dsm = (lds_char*)dsm_;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  const int nch = (M + 15) / 16;
  // W^T planes of output tiles 2 w + e: B[k = 32 ks + 8 g + j][col 16 (2 w + e) + c16] = W[col][k]
  bf16x8 bw[2][DS_KS][3];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int col = 16 * (2 * w + e) + c16;
#pragma unroll
    for (int ks = 0; ks < DS_KS; ++ks) {
      const int k0 = 32 * ks + 8 * g;
      f32x4 v0 = f32x4{0.f, 0.f, 0.f, 0.f}, v1 = v0;
      if (w < NT2 && col < KO && k0 < FG) {
        v0 = *reinterpret_cast<const f32x4*>(W + (size_t)col * FG + k0);
        v1 = *reinterpret_cast<const f32x4*>(W + (size_t)col * FG + k0 + 4);
      }
      uint32_t p0[3][2], p1[3][2];
      split3(v0, p0);
      split3(v1, p1);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        bw[e][ks][q] = __builtin_bit_cast(bf16x8, make_uint4(p0[q][0], p0[q][1], p1[q][0], p1[q][1]));
        // tile 1's planes live in the accumulator half of the register file (MFMA B operands may be
        // AGPRs): without the pin the compiler parks them there anyway and copies each one back to
        // VGPRs before its MFMA (4 v_accvgpr_read per MFMA)
        if (e == 1) asm volatile("" : "+a"(bw[e][ks][q]));
      }
    }
  }
  f32x4 v[DS4_NS][DS4_SLOTS];
  auto load = [&](auto S_, int c) {  // chunk c's rows (past M: zero-size descriptor, zeros)
    constexpr int S = decltype(S_)::value;
    const int r0 = c * 16, nr = c < nch ? min(16, M - r0) : 0;
    const rsrc_t rd = make_rsrc(reinterpret_cast<const char*>(D) + (nr ? (size_t)r0 * DRB : 0), nr * DRB);
#pragma unroll
    for (int j = 0; j < DS4_SLOTS; ++j) {
      const int e = tid + 256 * j, r = e / 100, c4 = e - 100 * r;
      v[S][j] = ld4(rd, e < 1600 ? (r * FG + 4 * c4) * 4 : kOOB);
    }
  };
  auto stage = [&](auto S_, lds_char* buf, int j) {
    constexpr int S = decltype(S_)::value;
    const int e = tid + 256 * j, r = e / 100, c4 = e - 100 * r;
    if (e >= 1600) return;
    const int lo = (r * DS4_RS + 4 * c4) * 2;
    split3_store(v[S][j], buf + lo, DS4_PL);
  };
  // zero the k = 400..415 pad columns of both buffers (never staged; the k-step 12 fragments read them)
  for (int i = tid; i < 2 * 3 * 16 * 2; i += 256) {
    const int h = i & 1, b = i / 96, q = (i / 32) % 3, r = (i / 2) % 16;
    *reinterpret_cast<__attribute__((address_space(3))) u32x4_t*>(dsm + b * DS4_BUF + q * DS4_PL +
                                                                  (r * DS4_RS + FG + 8 * h) * 2) = u32x4_t{0, 0, 0, 0};
  }
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  const int cs = gridDim.x;
  // prologue: this workgroup's chunk i (i = 0, 1, ...) lives in register set i % DS4_NS; chunk 0 staged
  // into buffer 0, chunks 1 .. DS4_NS - 1 in flight
  load(I0{}, blockIdx.x);
#pragma unroll
  for (int j = 0; j < DS4_SLOTS; ++j) stage(I0{}, dsm, j);
  load(I1{}, blockIdx.x + cs);
  __syncthreads();
  const int ao = (c16 * DS4_RS + 8 * g) * 2;  // this lane's A fragment: row c16, k = 8 g .. + 7 of a k-step
  // chunk cc (buffer S): chunk cc + 2 cs loaded into set S, the MFMAs on buffer S, chunk cc + cs (set
  // S ^ 1) split into buffer S ^ 1 in slices after the last DS4_SLOTS k-steps (unconditional: past
  // the end it stages zeros)
  auto chunk = [&](auto S_, int cc, int P) {  // S: register set of chunk cc, P: its LDS buffer
    constexpr int S = decltype(S_)::value, SN = (S + 1) % DS4_NS;  // SN: set of chunk cc + cs
    load(S_, cc + DS4_NS * cs);
    const lds_char* A_ = dsm + P * DS4_BUF;
    lds_char* nxt = dsm + (P ^ 1) * DS4_BUF;
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    // A fragments one k-step ahead (two sets): the LDS latency hides under the previous k-step's MFMAs
    bf16x8 af[2][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) af[0][q] = *reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>(A_ + q * DS4_PL + ao);
#pragma unroll
    for (int ks = 0; ks < DS_KS; ++ks) {
      __builtin_amdgcn_sched_barrier(0);
      if (ks + 1 < DS_KS) {
#pragma unroll
        for (int q = 0; q < 3; ++q)
          af[(ks + 1) & 1][q] = *reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>(A_ + q * DS4_PL + ao + 64 * (ks + 1));
      }
      const bf16x8(&a)[3] = af[ks & 1];
#pragma unroll
      for (int e = 0; e < 2; ++e) acc[e] = mma_split6(a, bw[e][ks], acc[e]);
      if (ks >= DS4_K0) {
        stage(std::integral_constant<int, SN>{}, nxt, ks - DS4_K0);  // (compile-time)
        // in-order issue: the split's VALU only overlaps the matrix pipe when it sits BETWEEN the
        // MFMAs in program order (12 MFMAs x 16 cycles vs ~24 VALU x 4 cycles per slot)
#pragma unroll
        for (int i = 0; i < 12; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
        }
      }
    }
    // output rows 16 cc + 4 g + i, columns 16 (2 w + e) + c16
    const int nr = min(16, M - 16 * cc);
    const rsrc_t rx = make_rsrc(X + (size_t)16 * cc * KO, nr * KO * 4);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int col = 16 * (2 * w + e) + c16;
      const bool ok = w < NT2 && col < KO;
#pragma unroll
      for (int i = 0; i < 4; ++i) st1(acc[e][i], rx, ok ? ((4 * g + i) * KO + col) * 4 : kOOB, 0);
    }
    __syncthreads();
  };
  int c = blockIdx.x;
  for (; c + cs < nch; c += 2 * cs) {
    chunk(I0{}, c, 0);
    chunk(I1{}, c + cs, 1);
  }
  if (c < nch) chunk(I0{}, c, 0);
}

// ------------------------------------------------------------------------------------------
// the split input gradient with MFMA and staging wave roles: lstmf_dgrad_roles_kernel
// ------------------------------------------------------------------------------------------
// lstmf_dgrad_s4_kernel gives every wave every job in program order, one wave per SIMD: nothing covers a
// wave's post-barrier A-fragment read, the MFMA drain before its output stores or its barrier wait, its
// __syncthreads() drains the dZ prefetch and the output stores (vmcnt(0)) once per chunk, and at KO <= 112
// wave 3's second tile is all padding (78 MFMAs per chunk on zero planes).  Here, as in
// lstmf_wgrad_roles_kernel, the jobs go to different waves, 8 per workgroup, two per SIMD:
//   MFMA waves 0..6: wave w owns the ONE output tile of columns 16 w .. 16 w + 15 for all 13 k-steps and
//     holds its three W^T planes in registers (156 VGPRs; no AGPR pin).  Per chunk: the A fragments from
//     the LDS image one k-step ahead, mma_split6 per k-step onto one accumulator that starts at zero, four
//     dword stores.  The tile index is a run-time (uniform) value: every MFMA wave runs the same
//     straight-line chunk body, columns >= KO store to kOOB.
//   staging wave 7 (the slot of s4's padding tile): the dZ stream.  A 16-row chunk is 1600 contiguous
//     float4 = 25 slots of 64 lanes.  The registers roll: slot j of the chunk due in the idle LDS buffer is
//     split there and its registers are at once reloaded with slot j of the chunk DR_D chunks later, so
//     DR_D whole chunks (25.6 KB each) per CU are always in flight.
//   Alone the staging wave is the bound (25 slots x 26 instructions; as fast as s4, no faster), so each MFMA
//     wave takes DR_SH of the 25 slots, each split between the MFMAs of one k-step, and the staging wave
//     keeps 25 - 7 DR_SH.  At DR_SH = 2 every SIMD stages 12 - 13 slots beside its MFMAs (SIMD 3: one
//     wave's 78 MFMAs and 2 + 11 slots; the others 156 MFMAs and 4 slots).  Measured at 6.3 M rows
//     (profiles/dgrad_roles): DR_SH / DR_D = 0/1 3.44, 1/1 3.35, 2/1 3.15, 3/1 3.25, 1/2 3.15, 2/2 3.04,
//     3/2 3.14 ms against s4's 3.46; the k-steps of the MFMA waves' slots and the staging wave at
//     s_setprio 1 are neutral.
// One lds_barrier() per chunk (LDS only: loads and stores stay in flight) separates "buffer P consumed"
// from "buffer P ^ 1 produced"; the role branch is taken once, outside the chunk loop.  LDS image, per-chunk
// descriptors from a 64-bit base (zero-size past M), chunk order (chunk i of workgroup b = b + i gridDim)
// and the arithmetic per output element -- k-steps 0..12 in order, mma_split6's six products chained onto a
// zero accumulator -- are those of s4: the result is bitwise that of lstmf_dgrad_s4_kernel.
#ifndef HFREP_DGRAD_ROLES_SHARE
#define HFREP_DGRAD_ROLES_SHARE 2  // DR_SH: staging slots (of 25) each MFMA wave takes, 0..3
#endif
#ifndef HFREP_DGRAD_ROLES_DEPTH
#define HFREP_DGRAD_ROLES_DEPTH 2  // DR_D: register sets of the dZ stream = chunks in flight per CU, 1 or 2
#endif
constexpr int DR_SH = HFREP_DGRAD_ROLES_SHARE, DR_D = HFREP_DGRAD_ROLES_DEPTH;
constexpr int DR_SLOTS = 16 * (FG / 4) / 64;  // 64-lane float4 slots per chunk (25)
constexpr int DR_NS = DR_SLOTS - 7 * DR_SH;   // slots of the staging wave
constexpr int DR_K0 = 2, DR_KST = 3;  // an MFMA wave's slot i goes between the MFMAs of k-step K0 + KST i
static_assert(DR_SH >= 0 && DR_SH <= 3 && (DR_D == 1 || DR_D == 2), "dgrad roles: share / depth");

__global__ void __launch_bounds__(512, 1)
lstmf_dgrad_roles_kernel(const float* __restrict__ D, const float* __restrict__ W, float* __restrict__ X, int M, int KO) {
  constexpr int DRB = 4 * FG;  // dZ row bytes
  extern __shared__ __attribute__((aligned(16))) char drm_[];
  lds_char* dsm = (lds_char*)drm_;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nch = (M + 15) / 16, cs = gridDim.x, cb = blockIdx.x;
  // zero the k = 400..415 pad columns of both buffers (never staged; the k-step 12 fragments read them)
  for (int i = tid; i < 2 * 3 * 16 * 2; i += 512) {
    const int h = i & 1, b = i / 96, q = (i / 32) % 3, r = (i / 2) % 16;
    *reinterpret_cast<__attribute__((address_space(3))) u32x4_t*>(dsm + b * DS4_BUF + q * DS4_PL +
                                                                  (r * DS4_RS + FG + 8 * h) * 2) = u32x4_t{0, 0, 0, 0};
  }
  // chunk c's rows (past M: zero-size descriptor, zeros); slot s of a chunk: float4 e = lane + 64 s of its
  // 1600, at byte 16 e of the chunk and at row e / 100, k = 4 (e % 100) of the image
  auto drsrc = [&](int c) {
    const int r0 = c * 16, nr = c < nch ? min(16, M - r0) : 0;
    return make_rsrc(reinterpret_cast<const char*>(D) + (nr ? (size_t)r0 * DRB : 0), nr * DRB);
  };
  auto slot_lo = [&](int s) {
    const int e = lane + 64 * s, r = e / 100;
    return (r * DS4_RS + 4 * (e - 100 * r)) * 2;
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  if (w < 7) {
    // ---------------- MFMA role ----------------
    const int g = lane >> 4, c16 = lane & 15, col = 16 * w + c16;
    // W^T planes of this wave's tile: B[k = 32 ks + 8 g + j][col] = W[col][k]
    // (columns >= KO and k >= 400 read zeros: offsets out of range, no branch)
    bf16x8 bw[DS_KS][3];
    const rsrc_t rw = make_rsrc(W, KO * FG * 4);
    int wrow = col * FG * 4;
#pragma unroll
    for (int ks = 0; ks < DS_KS; ++ks) {
      // one k-step's loads and split at a time: the next k-step's offset is made to depend on this one's
      // planes (all 26 loads hoisted ahead of the splits put the prologue past 256 registers)
      if (ks) asm volatile("" : "+v"(wrow), "+v"(bw[ks - 1][0]), "+v"(bw[ks - 1][1]), "+v"(bw[ks - 1][2]));
      const int k0 = 32 * ks + 8 * g, wo = col < KO && k0 < FG ? wrow + k0 * 4 : kOOB;
      const f32x4 v0 = ld4(rw, wo), v1 = ld4(rw, wo == kOOB ? kOOB : wo + 16);
      uint32_t p0[3][2], p1[3][2];
      split3(v0, p0);
      split3(v1, p1);
#pragma unroll
      for (int q = 0; q < 3; ++q) bw[ks][q] = __builtin_bit_cast(bf16x8, make_uint4(p0[q][0], p0[q][1], p1[q][0], p1[q][1]));
    }
    const int ao = (c16 * DS4_RS + 8 * g) * 2;  // this lane's A fragment: row c16, k = 8 g .. + 7 of a k-step
    // output rows 16 cc + 4 g + i, column 16 w + c16: byte offsets in the chunk's frame, kOOB for columns
    // >= KO.  (Opaque to the compiler: re-deriving the select per chunk put a branch between the last MFMA
    // and the stores of its result.)
    int xo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xo[i] = col < KO ? ((4 * g + i) * KO + col) * 4 : kOOB;
      asm volatile("" : "+v"(xo[i]));
    }
    // (share) this wave's DR_SH slots of the dZ stream: as the staging wave's, see below
    constexpr int NX = DR_SH ? DR_SH : 1;
    int xg[NX], xl[NX];
    f32x4 vx[DR_D][NX];
#pragma unroll
    for (int i = 0; i < DR_SH; ++i) {
      const int xs = DR_NS + DR_SH * w + i;
      xg[i] = 16 * (lane + 64 * xs);
      xl[i] = slot_lo(xs);
    }
#pragma unroll
    for (int s = 0; s < DR_D; ++s) {
      const rsrc_t rd = drsrc(cb + s * cs);
#pragma unroll
      for (int i = 0; i < DR_SH; ++i) vx[s][i] = ld4(rd, xg[i]);
    }
    {
      const rsrc_t rd = drsrc(cb + DR_D * cs);
#pragma unroll
      for (int i = 0; i < DR_SH; ++i) {
        split3_store(vx[0][i], dsm + xl[i], DS4_PL);
        vx[0][i] = ld4(rd, xg[i]);
      }
    }
    lds_barrier();
    // chunk cc in buffer P; chunk cc + cs (register set S) goes to buffer P ^ 1
    auto chunk = [&](auto P_, int cc) {
      constexpr int P = decltype(P_)::value, Q = P ^ 1, S = Q % DR_D;
      const lds_char* A_ = dsm + P * DS4_BUF + ao;
      const rsrc_t rdn = drsrc(cc + (1 + DR_D) * cs);
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
      // A fragments one k-step ahead (two sets): the LDS latency hides under the previous k-step's MFMAs
      bf16x8 af[2][3];
#pragma unroll
      for (int q = 0; q < 3; ++q) af[0][q] = *reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>(A_ + q * DS4_PL);
#pragma unroll
      for (int ks = 0; ks < DS_KS; ++ks) {
        __builtin_amdgcn_sched_barrier(0);
        if (ks + 1 < DS_KS) {
#pragma unroll
          for (int q = 0; q < 3; ++q)
            af[(ks + 1) & 1][q] = *reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>(A_ + q * DS4_PL + 64 * (ks + 1));
        }
        __builtin_amdgcn_sched_barrier(0);  // (the prefetch ahead of this k-step's MFMAs: a full k-step of lead)
        acc = mma_split6(af[ks & 1], bw[ks], acc);
        // slot i between the MFMAs of k-step DR_K0 + DR_KST i (in-order issue: the split's VALU only overlaps the
        // matrix pipe there), its reload in the next k-step: ahead of the output stores (vmcnt is in order
        // over loads and stores)
#pragma unroll
        for (int i = 0; i < DR_SH; ++i) {
          if (ks == DR_K0 + DR_KST * i) {
            split3_store(vx[S][i], dsm + Q * DS4_BUF + xl[i], DS4_PL);
#pragma unroll
            for (int n = 0; n < 6; ++n) {
              __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
              __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
            }
          }
          if (ks == DR_K0 + DR_KST * i + 1) vx[S][i] = ld4(rdn, xg[i]);
        }
      }
      const int nr = min(16, M - 16 * cc);
      const rsrc_t rx = make_rsrc(X + (size_t)16 * cc * KO, nr * KO * 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) st1(acc[i], rx, xo[i], 0);
      lds_barrier();
    };
    for (int cc = cb;;) {
      chunk(I0{}, cc);
      if ((cc += cs) >= nch) break;
      chunk(I1{}, cc);
      if ((cc += cs) >= nch) break;
    }
  } else {
    // ---------------- staging role ----------------
    int lo[DR_NS];
#pragma unroll
    for (int j = 0; j < DR_NS; ++j) lo[j] = slot_lo(j);
    // DR_D register sets: the workgroup's chunk i lives in set i % DR_D from DR_D chunk periods before it
    // is split into buffer i & 1.  roll(Q, c): the set of the chunk due in buffer Q is split there, each
    // slot reloaded with chunk c's (DR_D chunks later) as soon as it is consumed, so DR_D whole chunks
    // (25.6 KB each) stay in flight.  Unconditional: past the end zeros go to the idle buffer
    f32x4 v[DR_D][DR_NS];
    auto roll = [&](auto Q_, int c) {
      constexpr int Q = decltype(Q_)::value, S = Q % DR_D;
      const rsrc_t rd = drsrc(c);
#pragma unroll
      for (int j = 0; j < DR_NS; ++j) {
        split3_store(v[S][j], dsm + Q * DS4_BUF + lo[j], DS4_PL);
        v[S][j] = ld4(rd, 16 * (lane + 64 * j));
      }
    };
#pragma unroll
    for (int s = 0; s < DR_D; ++s) {
      const rsrc_t rd = drsrc(cb + s * cs);
#pragma unroll
      for (int j = 0; j < DR_NS; ++j) v[s][j] = ld4(rd, 16 * (lane + 64 * j));
    }
    roll(I0{}, cb + DR_D * cs);
    lds_barrier();
    // chunk cc (buffer P) is being consumed: chunk cc + cs into buffer P ^ 1
    for (int cc = cb;;) {
      roll(I1{}, cc + (1 + DR_D) * cs);
      lds_barrier();
      if ((cc += cs) >= nch) break;
      roll(I0{}, cc + (1 + DR_D) * cs);
      lds_barrier();
      if ((cc += cs) >= nch) break;
    }
  }
}

// ==========================================================================================
// fp32 input gradient dX = dZ W^T   (dZ: M x 400, W: KO x 400 row-major, dX: M x KO, KO <= 16 NT)
// ==========================================================================================
// hipBLASLt ran this product at 59 % (KO = 100) / 41 % (KO = 32) of the fp32 MFMA pipe on the
// 6.3 M-row calls of the B = 262k step (profiles/r02_final/kernel_summary_B262144_fp32.txt,
// MT112x256x32 / MT32x256x32), 11 % of the fp32 step.
//
// One persistent workgroup per CU, 4 waves (one per SIMD), each workgroup a contiguous range of
// 16-row chunks.  Wave w owns the k-slice [100 w, 100 w + 100) of the 400-long reduction for ALL NT
// output tiles: its W^T fragments (NT x 25 k-steps) live in registers and its A operand comes
// straight from HBM into registers — every dZ byte is loaded once, by one lane, no LDS staging.
// k is permuted inside the slice (k-step 4 q + j of lane group g reads k = 16 q + 4 g + j; step 24
// reads k = 96 + g), so a lane's four consecutive k-steps are one contiguous dwordx4 (the sum over
// k is order-free; A and B use the same map).  The four waves' partial tiles meet in LDS: chunk
// c's accumulators (two alternating register sets) are written during chunk c + 1's MFMAs and
// summed in fixed wave order during chunk c + 2's, so one barrier per chunk is the only stall.
constexpr int DG_KS = 25;
template <int NT>
__global__ void __launch_bounds__(256, 1)
lstmf_dgrad_kernel(const float* __restrict__ D, const float* __restrict__ W, float* __restrict__ X, int M, int KO,
                   int rows_per_wg) {
  __shared__ __attribute__((aligned(16))) f32x4 part[2][4][NT][64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  const int mb = blockIdx.x * rows_per_wg, nrows = min(M, mb + rows_per_wg) - mb;
  if (nrows <= 0) return;  // uniform over the workgroup
  const int kb = 100 * w;

  float bw[NT][DG_KS];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int col = 16 * n + c16;
#pragma unroll
    for (int s = 0; s < DG_KS; ++s) {
      const int k = s < 24 ? kb + 16 * (s >> 2) + 4 * g + (s & 3) : kb + 96 + g;
      bw[n][s] = col < KO ? W[col * FG + k] : 0.f;
    }
  }
  const rsrc_t rd = make_rsrc(D + (size_t)mb * FG, nrows * FG * 4);
  const rsrc_t rx = make_rsrc(X + (size_t)mb * KO, nrows * KO * 4);
  const int nch = (nrows + 15) / 16;

  f32x4 a0[6], a1[6], acc0[NT], acc1[NT];
  float s0 = 0.f, s1 = 0.f;
  auto load = [&](f32x4 (&a)[6], float& a_s, int r0) {
    const int vo = ((r0 + c16) * FG + kb + 4 * g) * 4;  // rows past the range read zeros
#pragma unroll
    for (int q = 0; q < 6; ++q) a[q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rd, vo + 64 * q, 0, 0));
    a_s = ld1(rd, vo + (96 - 3 * g) * 4, 0);
  };
  auto mm = [&](f32x4 (&acc)[NT], const f32x4 (&a)[6], int q0, int q1) {
#pragma unroll
    for (int q = q0; q < q1; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n] = mma4(a[q][j], bw[n][4 * q + j], acc[n]);
  };
  auto put = [&](const f32x4 (&acc)[NT], int slot) {
#pragma unroll
    for (int n = 0; n < NT; ++n) part[slot][w][n][lane] = acc[n];
  };
  // branch-free (a fixed number of stores on every path keeps the vmcnt waits of the MFMA operand
  // loads exact); invalid lanes / chunks store to kOOB
  auto reduce = [&](int slot, int r0, bool on) {
#pragma unroll
    for (int e = 0; e < (NT * 64 + 255) / 256; ++e) {
      const int idx = tid + 256 * e, ok = on && idx < NT * 64, ix = idx < NT * 64 ? idx : 0;
      const int n = ix >> 6, ln = ix & 63, col = 16 * n + (ln & 15), row = r0 + 4 * (ln >> 4);
      const f32x4 v = ((part[slot][0][n][ln] + part[slot][1][n][ln]) + part[slot][2][n][ln]) + part[slot][3][n][ln];
#pragma unroll
      for (int i = 0; i < 4; ++i) st1(v[i], rx, ok && col < KO ? ((row + i) * KO + col) * 4 : kOOB, 0);
    }
  };
  // chunk c: chunk c - 2's partials are reduced and stored FIRST (vmcnt is in order over loads and
  // stores: stores issued after the next chunk's loads would be waited for with them), then the
  // next chunk's A operands are loaded, then the MFMAs run into cur with chunk c - 1's
  // accumulators (prev) written to LDS under them
  auto chunk = [&](f32x4 (&cur)[NT], const f32x4 (&prev)[NT], const f32x4 (&a)[6], float a_s, f32x4 (&an)[6],
                   float& an_s, int c) {
    reduce(c & 1, 16 * (c - 2), c >= 2);
    load(an, an_s, 16 * (c + 1));  // past the end: out of range, zeros
    __builtin_amdgcn_sched_barrier(0);  // keep the loads ahead of the MFMAs (the scheduler sinks them)
#pragma unroll
    for (int n = 0; n < NT; ++n) cur[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    mm(cur, a, 0, 2);
    if (c >= 1) put(prev, (c - 1) & 1);
    mm(cur, a, 2, 6);
#pragma unroll
    for (int n = 0; n < NT; ++n) cur[n] = mma4(a_s, bw[n][24], cur[n]);
    __syncthreads();
  };

  // unrolled by two so the A-operand and accumulator sets alternate without register copies
  load(a0, s0, 0);
  int c = 0;
  for (; c + 2 <= nch; c += 2) {
    chunk(acc0, acc1, a0, s0, a1, s1, c);
    chunk(acc1, acc0, a1, s1, a0, s0, c + 1);
  }
  if (c < nch) chunk(acc0, acc1, a0, s0, a1, s1, c++);
  // drain (c == nch): the last chunk's accumulators, then the last two reductions
  if (c & 1)
    put(acc0, (c - 1) & 1);
  else
    put(acc1, (c - 1) & 1);
  reduce(c & 1, 16 * (c - 2), c >= 2);
  __syncthreads();
  reduce((c - 1) & 1, 16 * (c - 1), true);
}

// ==========================================================================================
// host side
// ==========================================================================================
bool lstmf_wgrad_supported(int K, int H, int N) { return H == FH && N == FG && (K == 32 || K == 35 || K == 36 || K == 100); }

// impl 1 / 2 / 3 / 4: the exact-fp32 MFMA kernel / the three-term bf16 split (pair) / the split quad /
// the split with MFMA and staging wave roles (pair partition at K = 32, quad partition at K = 100;
// bitwise equal to impl 2 / 3 there); default (0): exact under HFREP_FP32_EXACT, else the role kernel at
// K in {32, 100} and the pair split for K = 35 / 36 (profiles/r03_split, profiles/wgrad_roles)
static int wgradf_pick(int impl, int K) {
  int v = impl >= 1 && impl <= 4 ? impl : (fp32_exact() ? 1 : 0);
  if (K == 35 && v == 3) v = 2;  // the quad kernel reads 16-byte X rows only
  const bool roles = K == 32 || K == 100;  // the role kernel: K in {32, 100}
  if (v == 0) v = roles ? 4 : 0;
  if (v == 4 && !roles) v = 0;
  return v ? v : (K <= 36 ? 2 : 3);
}
// The partition of the M rows that kernel v (after wgradf_pick) runs on: np workgroups (column parts)
// share each of z row ranges of `rows` rows (a multiple of the kernel's chunk), np * z <= one workgroup per
// CU.  zcap >= z is the number of row ranges before `rows` is rounded up to whole chunks: the workspace
// holds zcap slabs (one per row range; the kernels write and the reduce reads the first z), so its size
// and the launch come from this one place.
// (The role kernel keeps the partition of the kernel it replaces: the pair's at K = 32, the quad's at 100.)
struct WgradPart {
  int np, z, rows, zcap;
};
static WgradPart wgradf_part(int v, int K, int M) {
  const int np = v == 1 ? 1 : v == 3 || (v == 4 && K == 100) ? 4 : 2;
  if (M <= 0) return {np, 0, 0, 0};
  const int ch = v == 1 ? WF_R : 32;
  const int chunks = (M + ch - 1) / ch, wgs = device_cu_count() / np;
  const int z0 = chunks < wgs ? chunks : wgs;
  const int rows = ((M + z0 - 1) / z0 + ch - 1) / ch * ch;
  return {np, (M + rows - 1) / rows, rows, z0};
}
size_t lstmf_wgrad_workspace_floats(int M, int K, int impl) {
  return (size_t)wgradf_part(wgradf_pick(impl, K), K, M).zcap * ((K == 35 ? 36 : K) + FH + 1) * FG;
}

bool launch_lstmf_wgrad(const float* X, const float* Hs, const float* D, const float* Xd, const float* Hds, const float* Dd,
                        float* gW, float* gU, float* gb, int M, int K, int Tn, float* ws, hipStream_t s, int impl) {
  if (!lstmf_wgrad_supported(K, FH, FG) || M <= 0) return false;
  const int v = wgradf_pick(impl, K);
  const WgradPart p = wgradf_part(v, K, M);
  auto go = [&](auto k, size_t sm) {  // the split kernels: dynamic LDS, (parts x row ranges) workgroups
    allow_lds(reinterpret_cast<const void*>(k));
    hipLaunchKernelGGL(k, dim3(p.np * p.z), dim3(512), sm, s, X, Hs, D, Xd, Hds, Dd, ws, M, Tn, p.rows, p.z);
  };
  auto exact = [&](auto k) { hipLaunchKernelGGL(k, dim3(p.z), dim3(512), 0, s, X, Hs, D, Xd, Hds, Dd, ws, M, Tn, p.rows); };
  switch (v * 128 + K) {
    case 1 * 128 + 32: exact(lstmf_wgrad_kernel<32>); break;
    case 1 * 128 + 35: exact(lstmf_wgrad_kernel<36, 35>); break;
    case 1 * 128 + 36: exact(lstmf_wgrad_kernel<36>); break;
    case 1 * 128 + 100: exact(lstmf_wgrad_kernel<100>); break;
    case 2 * 128 + 32: go(lstmf_wgrad_split_kernel<32>, 2 * WSGeo<32>::Img::BUF); break;
    case 2 * 128 + 35: go(lstmf_wgrad_split_kernel<36, 35>, 2 * WSGeo<36>::Img::BUF); break;
    case 2 * 128 + 36: go(lstmf_wgrad_split_kernel<36>, 2 * WSGeo<36>::Img::BUF); break;
    case 2 * 128 + 100: go(lstmf_wgrad_split_kernel<100>, 2 * WSGeo<100>::Img::BUF); break;
    case 3 * 128 + 32: go(lstmf_wgrad_q4_kernel<32>, 2 * WQGeo<32>::Img::BUF); break;
    case 3 * 128 + 36: go(lstmf_wgrad_q4_kernel<36>, 2 * WQGeo<36>::Img::BUF); break;
    case 3 * 128 + 100: go(lstmf_wgrad_q4_kernel<100>, 2 * WQGeo<100>::Img::BUF); break;
    case 4 * 128 + 32: go(lstmf_wgrad_roles_kernel<32>, 2 * WRGeo<32>::Img::BUF); break;
    case 4 * 128 + 100: go(lstmf_wgrad_roles_kernel<100>, 2 * WRGeo<100>::Img::BUF); break;
    default: throw std::runtime_error("lstmf_wgrad: no kernel for this impl / K");
  }
  launch_lstm_wgrad2_reduce(ws, gW, gU, gb, p.z, K, FH, FG, s, K == 35 ? 36 : K);
  return true;
}

bool lstmf_dgrad_supported(int N, int KO) { return N == FG && KO >= 1 && KO <= 16 * FNT; }

// impl 1 / 3 / 4: the exact-fp32 MFMA kernel / the LDS-staged split kernel lstmf_dgrad_s4_kernel / the
// split with MFMA and staging wave roles lstmf_dgrad_roles_kernel (bitwise equal to impl 3); default (0):
// exact under HFREP_FP32_EXACT, else the role kernel for KO > 64 and exact otherwise (the split kernels
// keep one wave busy per 16 / 32 output columns, so KO = 32 leaves most of the matrix pipe idle;
// profiles/r03_split, profiles/dgrad_roles).  s4 is reached by impl = 3 only: the reference of the tests.
bool launch_lstmf_dgrad(const float* D, const float* W, float* X, int M, int N, int KO, hipStream_t s, int impl) {
  if (!lstmf_dgrad_supported(N, KO) || M <= 0) return false;
  const int dv = impl == 1 || impl == 3 || impl == 4 ? impl : (fp32_exact() ? 1 : 0);
  if (dv == 4 || (dv == 0 && KO > 64)) {
    const int chunks = (M + 15) / 16, cus = device_cu_count();
    const int grid = chunks < cus ? chunks : cus;
    allow_lds(reinterpret_cast<const void*>(lstmf_dgrad_roles_kernel));
    hipLaunchKernelGGL(lstmf_dgrad_roles_kernel, dim3(grid), dim3(512), (size_t)2 * DS4_BUF, s, D, W, X, M, KO);
    return true;
  }
  if (dv == 3) {
    const int chunks = (M + 15) / 16, cus = device_cu_count();
    const int grid = chunks < cus ? chunks : cus;
    auto go = [&](auto k) {
      allow_lds(reinterpret_cast<const void*>(k));
      hipLaunchKernelGGL(k, dim3(grid), dim3(256), (size_t)2 * DS4_BUF, s, D, W, X, M, KO);
    };
    switch ((KO + 31) / 32) {
      case 1: go(lstmf_dgrad_s4_kernel<1>); break;
      case 2: go(lstmf_dgrad_s4_kernel<2>); break;
      case 3: go(lstmf_dgrad_s4_kernel<3>); break;
      default: go(lstmf_dgrad_s4_kernel<4>); break;
    }
    return true;
  }
  // one workgroup per CU (two for NT <= 3: HBM-bound there, and the registers allow a second one
  // in flight); more only if a workgroup's dZ range would pass 2 GB (32-bit buffer offsets)
  const int chunks = (M + 15) / 16, cus = device_cu_count() * (KO <= 48 ? 2 : 1);
  int grid = chunks < cus ? chunks : cus;
  const int min_grid = (int)(((long long)M * FG * 4 + (1ll << 31) - 1) / (1ll << 31));
  if (grid < min_grid) grid = min_grid;
  const int rpw = (chunks + grid - 1) / grid * 16;
  const int z = (M + rpw - 1) / rpw;
  switch ((KO + 15) / 16) {
    case 1: hipLaunchKernelGGL(lstmf_dgrad_kernel<1>, dim3(z), dim3(256), 0, s, D, W, X, M, KO, rpw); break;
    case 2: hipLaunchKernelGGL(lstmf_dgrad_kernel<2>, dim3(z), dim3(256), 0, s, D, W, X, M, KO, rpw); break;
    case 3: hipLaunchKernelGGL(lstmf_dgrad_kernel<3>, dim3(z), dim3(256), 0, s, D, W, X, M, KO, rpw); break;
    case 4: hipLaunchKernelGGL(lstmf_dgrad_kernel<4>, dim3(z), dim3(256), 0, s, D, W, X, M, KO, rpw); break;
    case 5: hipLaunchKernelGGL(lstmf_dgrad_kernel<5>, dim3(z), dim3(256), 0, s, D, W, X, M, KO, rpw); break;
    case 6: hipLaunchKernelGGL(lstmf_dgrad_kernel<6>, dim3(z), dim3(256), 0, s, D, W, X, M, KO, rpw); break;
    default: hipLaunchKernelGGL(lstmf_dgrad_kernel<7>, dim3(z), dim3(256), 0, s, D, W, X, M, KO, rpw); break;
  }
  return true;
}

}  // namespace hfrep
