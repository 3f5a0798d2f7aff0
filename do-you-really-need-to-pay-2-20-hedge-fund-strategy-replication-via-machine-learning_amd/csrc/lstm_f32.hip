// fp32 LSTM layer kernels (gfx950): exact-fp32 MFMA, fused input projection, persistent.
//
// The fp32 (reference-precision) path used to run the v1 recurrences of lstm.hip on a zx = x W + b
// tensor materialised by a separate GEMM: at B = 32k that GEMM alone wrote 1.3 GB per layer call and
// the v1 recurrence issued its zx loads at the top of every step (profiles/r02_prof_fp32: the
// linear / wgrad GEMMs were 60 % and the recurrences 37 % of the fp32 step).  In fp32 the matrix
// pipe is the bound (v_mfma_f32_16x16x4_f32: 64 FLOP/clk/SIMD, 1/16 of bf16), so this design is
// about keeping MFMA issue dense and the padding small:
//
//  * 4 waves per workgroup, ONE per SIMD (~400 VGPRs each), one persistent workgroup per CU walking
//    32-row tiles.  Wave w owns units 28 w .. 28 w + 27 (100 units -> 7 + 7 + 7 + 4 tiles of 4 units;
//    12 % padding instead of the 28 % of 32-unit waves);
//  * GATE-INTERLEAVED 16-column MFMA tiles: column c of tile n is gate (c & 3) of unit
//    28 w + 4 n + (c >> 2), so the four gates of a unit sit in one lane quad.  Each lane applies
//    its own gate's nonlinearity to its 4 accumulator rows (no lane computes a gate it does not
//    own), then a 4 x 4 quad transpose (DPP quad_perm) gives every lane the i, f, g, o of ONE
//    (row, unit) for the cell update: no redundant transcendentals and a 1-register cell state;
//  * U^T fragments in registers (25 k-steps x 7 tiles), W^T fragments in registers for the first
//    12 k-steps and in LDS for the rest (K = 100: 93 KB), so z_t = x_t W + h_{t-1} U + b is one
//    MFMA chain per tile and zx never exists in HBM;
//  * A operands (x_t, h_{t-1}) in LDS in a K-permuted layout (element k at (k & 3) * KQ + (k >> 2)
//    of its row) so one ds_read_b128 feeds four 16x16x4 k-steps; the row strides are chosen
//    conflict-free for ds_read_b128 (scripted search over the CDNA4 lane groups);
//  * x_{t+1} is loaded into registers at the top of step t and written to LDS at its end, so its
//    HBM latency hides under the step's ~700 MFMAs;
//  * outputs in the row-major layouts of the v1 contract (h (B,T,H), gate activations (B,T,4H),
//    cells (B,T,H); the tangent's hdot, zdot, cdot), so the v1 reverse kernels consume them.
//
// At K = 100 (the second layer of both models) the forward runs on eight waves, two per SIMD, by default:
// lstmf_fwd2_kernel regroups the 25 real tiles (8 x 3, tile 24 split by row half between waves 0 and 1, no
// padding tiles: 13 / 13 / 12 / 12 tile-halves per SIMD), keeps U^T in registers and
// most of W^T in LDS, and runs one wave's gate math under its SIMD partner's MFMA chain; its outputs are bitwise
// lstmf_fwd_kernel's (set_lstmf_fwd100_impl: 1 four waves, 2 eight waves; profiles/fwd100_two_wave/README.md).
// lstmf_fwd_kernel stays as that reference, for K = 32 / 35 / 36 under forward impl 1 and for the K = 35 / 36
// tangent forwards.
//
// TAN = true is the tangent forward at a saved primal point (ops/reference.py lstm_seq_tfwd with
// dzx = xd W folded in): zdot_t = xd_t W + hdot_{t-1} U, primal gates / cells read from the tape.
//
// The four reverse kernels (lstmf_bwdp / lstmf_bwds: BPTT exact / split; lstmf_tbwdp / lstmf_tbwd1: tangent
// reverse with two streams / one) take the dZ store share, the exact MFMA role, the BPTT cell adjoint, the
// tangent step loads, the HEAD row factors and the padded-unit mask from one definition each ("stages the
// reverse kernels share", above the kernels); the tangent cell adjoint is a helper in lstmf_tbwdp and
// written out in lstmf_tbwd1, whose bits it would change.
// lstmf_bwds2 is lstmf_bwds on eight waves, two per SIMD (seven tile waves and one wave with the dZ stores; same
// bits): the default BPTT where no h adjoints are kept (set_lstmf_bwd_impl 4; profiles/bwds_two_wave/README.md).
#include "lstmf_dev.h"

#include <atomic>
#include <cstdlib>
#include <type_traits>
#include <stdexcept>

namespace hfrep {

namespace {

// rows [row0, row0 + 32) (clipped to B) of a row-major (B, Tn, W) fp32 tensor
__device__ __forceinline__ rsrc_t ftile_rsrc(const float* base, int row0, int B, int Tn, int W) {
  row0 = __builtin_amdgcn_readfirstlane(row0);
  const int nr = base ? max(0, min(32, B - row0)) : 0;
  return make_rsrc(base + (nr ? (size_t)row0 * Tn * W : 0), nr * Tn * W * 4);
}

// geometry of a K-wide A operand tile (32 rows) in LDS: KS k-steps of 4; element k of a row at
// (k & 3) * KQ + (k >> 2); row stride LR.  (KQ, LR) = (12, 56) / (28, 120) are conflict-free for the
// ds_read_b128 fragment reads (lane l: row l & 15, k-group l >> 4) over all four lane groups.
template <int K>
struct FGeo {
  static_assert(K >= 1 && K <= 112, "fp32 LSTM: K <= 112");
  static constexpr int KS = (K + 3) / 4;
  static constexpr int KQ = KS <= 12 ? 12 : 28;
  static constexpr int LR = KS <= 12 ? 56 : 120;
  static constexpr int NJ = (KS + 3) / 4;  // b128 reads per row
};
// W^T k-steps kept in registers (the rest live in LDS)
template <int K>
constexpr int f_nwr() { return FGeo<K>::KS <= 12 ? FGeo<K>::KS : 12; }
template <int K>
constexpr int f_nwl() { return FGeo<K>::KS - f_nwr<K>(); }

// quad_perm DPP moves (lane q of each quad reads lane perm[q])
__device__ __forceinline__ float qswap2(float v) {  // [2,3,0,1]
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
}
__device__ __forceinline__ float qswap1(float v) {  // [1,0,3,2]
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
}
// 4 x 4 transpose inside each lane quad: lane q holds a[i] = M[q][i]; afterwards a[k] = M[k][q]
__device__ __forceinline__ void quad_transpose(float (&a)[4], int q) {
  const float p0 = qswap2(a[0]), p1 = qswap2(a[1]), p2 = qswap2(a[2]), p3 = qswap2(a[3]);
  const bool lo = q < 2;
  const float b0 = lo ? a[0] : p2, b1 = lo ? a[1] : p3, b2 = lo ? p0 : a[2], b3 = lo ? p1 : a[3];
  const float r0 = qswap1(b0), r1 = qswap1(b1), r2 = qswap1(b2), r3 = qswap1(b3);
  const bool ev = !(q & 1);
  a[0] = ev ? b0 : r1;
  a[1] = ev ? r0 : b1;
  a[2] = ev ? b2 : r3;
  a[3] = ev ? r2 : b3;
}

// x tile loader: this thread's share of the 32 x K tile of one step, loaded to registers and
// written to the K-permuted LDS layout.  Offsets are computed once per row block.
template <int K>
struct FXPart {
  static constexpr bool VEC = K % 4 == 0;
  static constexpr int PER = VEC ? K / 4 : K;                 // chunks per row
  static constexpr int NJ = (32 * PER + 255) / 256;
  float v[VEC ? 4 * NJ : NJ];
  int goff[NJ], lpos[NJ];
  __device__ __forceinline__ void set(int Tn, int tid) {
    using GX = FGeo<K>;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int e = tid + 256 * j, r = e / PER, c = e - r * PER;
      const bool ok = r < 32;
      if constexpr (VEC) {
        goff[j] = ok ? (r * Tn * K + 4 * c) * 4 : kOOB;
        lpos[j] = ok ? r * GX::LR + c : -1;
      } else {
        goff[j] = ok ? (r * Tn * K + c) * 4 : kOOB;
        lpos[j] = ok ? r * GX::LR + (c & 3) * GX::KQ + (c >> 2) : -1;
      }
    }
  }
  __device__ __forceinline__ void load(rsrc_t rx, int Tn, int t, bool on) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int vo = on ? goff[j] : kOOB;
      if constexpr (VEC) {
        const f32x4 d = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, vo, t * K * 4, 0));
        v[4 * j] = d[0]; v[4 * j + 1] = d[1]; v[4 * j + 2] = d[2]; v[4 * j + 3] = d[3];
      } else {
        v[j] = ld1(rx, vo, t * K * 4);
      }
    }
  }
  __device__ __forceinline__ void to_lds(float* xb, float* trash) const {
    using GX = FGeo<K>;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      float* d = lpos[j] >= 0 ? xb + lpos[j] : trash;
      if constexpr (VEC) {
        const int s = lpos[j] >= 0 ? GX::KQ : 0;
        d[0] = v[4 * j]; d[s] = v[4 * j + 1]; d[2 * s] = v[4 * j + 2]; d[3 * s] = v[4 * j + 3];
      } else {
        d[0] = v[j];
      }
    }
  }
};

// fp32 tape: a lane-native blocked layout.  Per (32-row block, step) and per wave w and accumulator
// pair (m, n) one SLOT of 64 lanes x {4 gate values (16 bytes), 1 cell value}: the lane that computed
// the (row, unit) in the forward reads it back in the reverse kernels, and every wave-level access is
// a contiguous 1 KiB (gates) or 256 B (cell).  Primal tape: gate activations (i, f, g, o) and c_t;
// tangent tape: the gate pre-activation tangents zdot and cdot.  Slots of wave 3's padding tiles
// (units 100..111) are never written nor read.
constexpr int FT_MN = 2 * FNT, FT_SLOT = 64 * 5, FT_STEP = 4 * FT_MN * FT_SLOT;
__device__ __forceinline__ rsrc_t ftape_rsrc(const float* tape, int rb, int nrb, int Tn) {
  rb = __builtin_amdgcn_readfirstlane(rb);
  const bool on = tape && rb < nrb;
  return make_rsrc(tape + (on ? (size_t)rb * Tn * FT_STEP : 0), on ? Tn * FT_STEP * 4 : 0);
}
// byte offset of this lane's gate quad in slot (w, m, n) at step 0; the cell value is at +1024 - 12 lane
__device__ __forceinline__ int ftape_lane(int w, int lane) { return (w * FT_MN * FT_SLOT) * 4 + lane * 16; }
__device__ __forceinline__ int ftape_cell(int w, int lane) { return (w * FT_MN * FT_SLOT + 256 + lane) * 4; }
__device__ __forceinline__ constexpr int ftape_slot(int m, int n) { return (m * FNT + n) * FT_SLOT * 4; }

}  // namespace

// ==========================================================================================
// forward / tangent forward
// ==========================================================================================
template <int ACT, int KX, bool TAPE, bool TAN>
__global__ void __launch_bounds__(256, 1)
lstmf_fwd_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                 const float* __restrict__ U, const float* __restrict__ ptape, float* __restrict__ hs,
                 float* __restrict__ tape, int B, int Tn) {
  using GX = FGeo<KX>;
  using GH = FGeo<FH>;
  constexpr int NWR = f_nwr<KX>(), NWL = f_nwl<KX>();
  extern __shared__ __attribute__((aligned(16))) float fsm[];
  float* xb = fsm;                     // [2][32 * LRX]
  float* hb = xb + 2 * 32 * GX::LR;    // [2][32 * LRH]
  float* wl = hb + 2 * 32 * GH::LR;    // [NWL][4 waves][7 tiles][64 lanes]
  float* trash = wl + NWL * 4 * FNT * 64;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = lane & 3, g = lane >> 4, j4 = (lane & 15) >> 2;
  const int ub = FUW * w + j4;  // unit of tile 0 in this lane's MFMA column; tile n adds 4 n
  const int nrb = (B + 31) / 32;

  for (int i = tid; i < 2 * 32 * (GX::LR + GH::LR); i += 256) fsm[i] = 0.f;

  // ---- weight fragments (B operand of 16x16x4: lane l holds B[k = 4 ks + (l >> 4)][col l & 15]) ----
  constexpr float GSC = ACT == ACT_TANH ? -2.f * kLog2e : ACT == ACT_SIGMOID ? -kLog2e : 1.f;
  const float sc = TAN ? 1.f : (q == 2 ? GSC : -kLog2e);
  float uf[GH::KS][FNT];
  float wf[NWR][FNT];
  float bq[FNT];
#pragma unroll
  for (int n = 0; n < FNT; ++n) {
    const int u = ub + 4 * n;
    const bool ok = u < FH;
    const int cl = q * FH + (ok ? u : FH - 1);
#pragma unroll
    for (int ks = 0; ks < GH::KS; ++ks) {
      const float v = U[(4 * ks + g) * FG + cl];  // k = 4 ks + g < 100 always
      uf[ks][n] = ok ? v * sc : 0.f;
      // U^T lives in the accumulator half of the register file (MFMA B operands may be AGPRs):
      // the VGPR half stays free for W^T, the loads in flight and the gate math
      asm volatile("" : "+a"(uf[ks][n]));
    }
#pragma unroll
    for (int ks = 0; ks < GX::KS; ++ks) {
      const int k = 4 * ks + g;
      const float v = W[min(k, KX - 1) * FG + cl];
      const float wv = (ok && k < KX) ? v * sc : 0.f;
      if (ks < NWR) {
        wf[ks < NWR ? ks : 0][n] = wv;
        if (ks >= 8) asm volatile("" : "+a"(wf[ks < NWR ? ks : 0][n]));  // (K = 100: 4 of its 12 k-steps)
      }
      else wl[(((ks - NWR) * 4 + w) * FNT + n) * 64 + lane] = wv;
    }
    const float bv = bias ? bias[cl] : 0.f;
    bq[n] = (!TAN && ok) ? bv * sc : 0.f;
  }
  // per-lane gate nonlinearity y = lin ? s : am * rcp(1 + exp2(s)) + bm (pre-scaled s)
  const bool glin = !TAN && ACT == ACT_LINEAR && q == 2;
  const float am = (ACT == ACT_TANH && q == 2) ? 2.f : 1.f, bm = (ACT == ACT_TANH && q == 2) ? -1.f : 0.f;
  // LDS element offsets: A-fragment reads (row l & 15, k-group g) and the h write of (row 4 g + q, unit ub + 4 n)
  const int ax = (lane & 15) * GX::LR + g * GX::KQ, ah = (lane & 15) * GH::LR + g * GH::KQ;
  const int hw = (4 * g + q) * GH::LR + j4 * GH::KQ + 7 * w;

  for (int rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int row0 = rb * 32;
    const rsrc_t rx = ftile_rsrc(x, row0, B, Tn, KX);
    const rsrc_t rh = ftile_rsrc(hs, row0, B, Tn, FH);
    const rsrc_t rt = ftape_rsrc(TAPE ? tape : nullptr, rb, nrb, Tn);  // primal (or tangent) tape out
    const rsrc_t rp = ftape_rsrc(TAN ? ptape : nullptr, rb, nrb, Tn);  // tangent: the primal tape
    // byte offsets at step 0 of this lane's (row 16 m + 4 g + q, unit ub) in (B,T,H) (the descriptor
    // covers rows < B only, so a row past B is out of range by itself); every offset below is
    // (base + t * step stride) + an immediate, so nothing per tile is hoisted out of the step loop
    int vp1[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) vp1[m] = ((16 * m + 4 * g + q) * Tn * FH + ub) * 4;
    const int tl = ftape_lane(w, lane), tcl = ftape_cell(w, lane);
    float cprev[TAN ? 2 : 1][FNT];  // tangent: c_{t-1} of the primal (carried)
    if constexpr (TAN) {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < FNT; ++n) cprev[m][n] = 0.f;
    }
    float cst[2][FNT];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < FNT; ++n) cst[m][n] = 0.f;
    FXPart<KX> xp;
    xp.set(Tn, tid);
    xp.load(rx, Tn, 0, true);
    for (int i = tid; i < 32 * GH::LR; i += 256) hb[i] = 0.f;  // h_{-1} = 0
    xp.to_lds(xb, trash);
    __syncthreads();
    for (int t = 0; t < Tn; ++t) {
      const float* xcur = xb + (t & 1) * 32 * GX::LR;
      const float* hcur = hb + (t & 1) * 32 * GH::LR;
      float* hnext = hb + ((t + 1) & 1) * 32 * GH::LR;
      xp.load(rx, Tn, t + 1, t + 1 < Tn);  // x_{t+1}: lands during this step's MFMAs
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        // tangent: the primal gates and c_t of this lane's (row, unit), from its own tape slots;
        // issued before this half's MFMAs, consumed after them
        f32x4 pg[TAN ? FNT : 1];
        float pc[TAN ? FNT : 1];
        const int p1 = vp1[m] + t * FH * 4, tb = t * FT_STEP * 4;
        if constexpr (TAN) {
#pragma unroll
          for (int n = 0; n < FNT; ++n) {
            const bool tok = !(w == 3 && n >= 4);
            pg[n] = ld4(rp, tok ? tl + tb + ftape_slot(m, n) : kOOB);
            pc[n] = ld1(rp, tok ? tcl + tb + ftape_slot(m, n) : kOOB, 0);
          }
        }
        f32x4 acc[FNT];
#pragma unroll
        for (int n = 0; n < FNT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};  // (inline-constant C; bias added below)
        // ---- z = x_t W (+ b) ----
#pragma unroll
        for (int j = 0; j < GX::NJ; ++j) {
          const f32x4 a4 = *reinterpret_cast<const f32x4*>(xcur + ax + 16 * m * GX::LR + 4 * j);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int ks = 4 * j + s;
            if (ks >= GX::KS) break;
#pragma unroll
            for (int n = 0; n < FNT; ++n) {
              const float bw = ks < NWR ? wf[ks < NWR ? ks : 0][n] : wl[(((ks - NWR) * 4 + w) * FNT + n) * 64 + lane];
              acc[n] = mma4(a4[s], bw, acc[n]);
            }
          }
          __builtin_amdgcn_sched_barrier(0);  // bound the live range of hoisted fragment reads
        }
        // ---- + h_{t-1} U ----
#pragma unroll
        for (int j = 0; j < GH::NJ; ++j) {
          const f32x4 a4 = *reinterpret_cast<const f32x4*>(hcur + ah + 16 * m * GH::LR + 4 * j);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int ks = 4 * j + s;
            if (ks >= GH::KS) break;
#pragma unroll
            for (int n = 0; n < FNT; ++n) acc[n] = mma4(a4[s], uf[ks][n], acc[n]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        // ---- gate math, cell update, stores (row 16 m + 4 g + q, unit ub + 4 n after the transpose) ----
#pragma unroll
        for (int n = 0; n < FNT; ++n) {
          const bool tok = !(w == 3 && n >= 4);  // wave 3's tiles 4..6 are padding units 100..111
          const int v1 = tok ? p1 + 16 * n : kOOB;
          float hv;
          if constexpr (!TAN) {
            float y[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float s = acc[n][i] + bq[n];
              const float e = am * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(s)) + bm;
              y[i] = glin ? s : e;
            }
            quad_transpose(y, q);  // y = (i, f, g, o) of (row, unit)
            const float cn = y[1] * cst[m][n] + y[0] * y[2];
            float ca;
            if constexpr (ACT == ACT_TANH) ca = 2.f * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(GSC * cn)) - 1.f;
            else if constexpr (ACT == ACT_SIGMOID) ca = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(GSC * cn));
            else ca = cn;
            hv = tok ? y[3] * ca : 0.f;
            cst[m][n] = cn;
            if constexpr (TAPE) {
              st4(f32x4{y[0], y[1], y[2], y[3]}, rt, tok ? tl + tb + ftape_slot(m, n) : kOOB);
              st1(cn, rt, tok ? tcl + tb + ftape_slot(m, n) : kOOB, 0);
            }
          } else {
            // zdot of (row, unit) for all four gates: transpose the accumulator quad
            float zd[4] = {acc[n][0], acc[n][1], acc[n][2], acc[n][3]};
            quad_transpose(zd, q);
            const f32x4 y = pg[n];
            const float idot = y[0] * (1.f - y[0]) * zd[0], fdot = y[1] * (1.f - y[1]) * zd[1];
            const float gdot = act_dy(ACT, y[2]) * zd[2], odot = y[3] * (1.f - y[3]) * zd[3];
            const float c = pc[n];
            float cdn = fdot * cprev[m][n] + y[1] * cst[m][n] + idot * y[2] + y[0] * gdot;
            const float ca = act_f(ACT, c);
            float hd = odot * ca + y[3] * act_dy(ACT, ca) * cdn;
            if (!tok) { cdn = 0.f; hd = 0.f; }
            cst[m][n] = cdn;
            cprev[m][n] = c;
            hv = hd;
            st4(f32x4{zd[0], zd[1], zd[2], zd[3]}, rt, tok ? tl + tb + ftape_slot(m, n) : kOOB);
            st1(cdn, rt, tok ? tcl + tb + ftape_slot(m, n) : kOOB, 0);
          }
          hnext[hw + 16 * m * GH::LR + n] = hv;  // padded units (u < 112) write their zeros
          st1(hv, rh, v1, 0);
        }
      }
      xp.to_lds(xb + ((t + 1) & 1) * 32 * GX::LR, trash);
      lds_barrier();
    }
  }
}

// ==========================================================================================
// BPTT (fp32): dZ_t = dL/dz_t (ops/reference.py lstm_seq_bwd) from the row-major fp32 tapes
// ==========================================================================================
// Same wave / lane decomposition as the forward: after the quad transpose lane (g, j4, q) of wave
// w owns (row 16 m + 4 g + q, unit 28 w + 4 n + j4) for m < 2, n < 7, and keeps that cell's dc.
// Per step, two phases between LDS barriers:
//   A. dh_rec = dz_{t+1} U^T on 16x16x4 MFMAs: A = the dz tile in LDS (k = 4 u' + q, row layout
//      [q][u'] so one ds_read_b128 feeds four k-steps), B = U^T fragments pinned in AGPRs; wave w
//      owns output column tiles 2 w, 2 w + 1 (16 units each) for both row halves (400 MFMAs), and
//      the step's tape / dH loads are issued before it so their latency hides under the MFMAs;
//   B. the cell adjoint math per (row, unit), dZ_t to HBM (row-major, for the weight gradient and the
//      input-gradient GEMM) and to the dz tile for the next step.
constexpr int BZ_KQ = 100, BZ_LR = 408, BH_LR = 116;  // dz tile: conflict-free b128 reads (scripted search)

// dZ_{t+1} leaves through 16-byte row-major stores read back from the dz tile during phase A of step
// t (the tile holds it anyway), and step t-1's tape loads are issued at the end of phase B of step t,
// reusing the registers just consumed: every load is older than the stores it could queue behind
// (vmcnt retires loads and stores in issue order), and every store is coalesced.
// step t's tape for the BPTT: the gate quad at t and c_{t-1} (c_t is carried from the step above)
__device__ __forceinline__ void bwdf_tape_load(f32x4& tg, float& tcp, float& tdh, rsrc_t rt, rsrc_t rdh, int og, int ocp,
                                               int p1, bool tok, bool prev) {
  tg = ld4(rt, tok ? og : kOOB);
  tcp = ld1(rt, (tok && prev) ? ocp : kOOB, 0);
  tdh = ld1(rdh, tok ? p1 : kOOB, 0);
}
// the same loads with the per-lane part of each offset in voffset (tl / tcl / vp) and the uniform part
// (step and slot) in soffset: no per-cell offset arithmetic on the VALU (the split BPTT is VALU-bound,
// profiles/r03_end/pmc_fp32.txt).  Out-of-range lanes: voffset kOOB (the range check is on voffset)
// HEAD: dH is the critic head's outer-product adjoint dH[b, t, u] = hdm * w[t, u] (hdm = the lane row's
// d[b], w = the head weight, (Tn, H) like one row of dH: same soffset, voffset hvo = the unit's
// offset), generated here instead of read from a materialised (B, Tn, H) tensor
template <bool HEAD>
__device__ __forceinline__ void bwdf_tape_load_u(f32x4& tg, float& tcp, float& tdh, rsrc_t rt, rsrc_t rdh, int tl, int tcl,
                                                 int vp, int sg, int sc, int sd, bool tok, bool prev, float hdm,
                                                 rsrc_t rhw, int hvo) {
  tg = ld4s(rt, tok ? tl : kOOB, sg);
  tcp = ld1(rt, (tok && prev) ? tcl : kOOB, sc);
  // (the product may contract into the consumer's add: one rounding fewer than a materialised dH, i.e.
  // within an ulp of it; an empty-asm barrier against that breaks the step schedule, +40 % per call)
  if constexpr (HEAD) tdh = hdm * ld1(rhw, tok ? hvo : kOOB, sd);
  else tdh = ld1(rdh, tok ? vp : kOOB, sd);
}
// ------------------------------------------------------------------------------------------
// stages the reverse kernels share (lstmf_bwdp / lstmf_tbwdp / lstmf_tbwd1 / lstmf_bwds_kernel): one
// definition of the dZ store mapping, the exact MFMA role, the BPTT and the tangent cell adjoint, the tangent
// step loads, the HEAD row factors and the padded-unit mask.  Where a kernel keeps a written-out form, a
// comment at that site names the measurement (profiles/lstmf_rev_shared/README.md)
// ------------------------------------------------------------------------------------------
using I0 = std::integral_constant<int, 0>;
using I1 = std::integral_constant<int, 1>;
// wave 3's unit tiles 4..6 are the padding units 100..111: their cells read nothing, carry zeros and write
// to the trash row
__device__ __forceinline__ bool unit_ok(int w, int n) { return !(w == 3 && n >= 4); }

// the dz tile (32 rows x [q][u'], u' < 100) -> dZ[:, t, :] (row-major, 4H per row) in 16-byte chunks:
// threads 0..199 (of a role) own chunk (tid % 100) of rows 2 k + tid / 100 (k < 16); the row step lives in
// the uniform offset, so a thread holds one LDS and one global base (rows past B: voffset out of range)
struct RevStore {
  int lo, go, rr;
  __device__ __forceinline__ RevStore(int tid, int Tn) {
    rr = tid / 100;
    const int ch = tid - 100 * rr, qq = ch / 25, c = ch - 25 * qq;
    lo = (rr & 1) * BZ_LR + qq * BZ_KQ + 4 * c;
    go = tid < 200 ? (rr * Tn * FG + qq * FH + 4 * c) * 4 : kOOB;
  }
  // rows of half M of `tile` (holding dz at step ts) -> dZ[:, ts, :]; a half's rows are stable for exactly
  // the half-phase after the one that completed them.  SB: one schedule region per pair of rows (where the
  // stores ride on an MFMA role, ahead of its MFMAs)
  template <int M, bool SB>
  __device__ __forceinline__ void half(const float* tile, rsrc_t rz, int Tn, int ts, int nr) const {
#pragma unroll
    for (int k = 8 * M; k < 8 * M + 8; ++k) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(tile + lo + 2 * k * BZ_LR);
      st16(v, rz, 2 * k + rr < nr, go, (2 * k * Tn + ts) * FG * 4);
      if constexpr (SB) {
        if (k & 1) __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
};

// ---- the exact MFMA role (waves 0..3 of the role-split kernels): tile U^T on v_mfma_f32_16x16x4_f32 ----
// U^T fragments of wave w's output column tiles 2 w, 2 w + 1 (16 units each; arch VGPRs: at two waves per
// SIMD the role fits in 256 with U^T taking 200)
__device__ __forceinline__ void rev_ut_load(float (&ut)[2][FH], const float* __restrict__ U, int w, int c16, int g) {
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int j = 16 * (2 * w + e) + c16;
    const bool ok = j < FH;
#pragma unroll
    for (int k = 0; k < FH; ++k) {
      const float v = U[(ok ? j : 0) * FG + g * FH + k];
      ut[e][k] = ok ? v : 0.f;
    }
  }
}
// rows 16 M .. 16 M + 15 of tile U^T (tile: a dz-style tile, [q][u'] per row) -> the same rows of the
// dh-style tile `out`; a schedule barrier after every SB b128 fragment reads
template <int M, int SB>
__device__ __forceinline__ void rev_half_a(const float* tile, float* out, const float (&ut)[2][FH], int w, int c16, int g) {
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  const float* ar = tile + (16 * M + c16) * BZ_LR + g * BZ_KQ;
#pragma unroll
  for (int jj = 0; jj < FH / 4; ++jj) {
    const f32x4 a4 = *reinterpret_cast<const f32x4*>(ar + 4 * jj);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      acc[0] = mma4(a4[s], ut[0][4 * jj + s], acc[0]);
      acc[1] = mma4(a4[s], ut[1][4 * jj + s], acc[1]);
    }
    if (jj % SB == SB - 1) __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int col = 16 * (2 * w + e) + c16;
    if (2 * w + e < 7) {  // (wave 3's second tile is past the 112-unit tile: uniform skip)
#pragma unroll
      for (int i = 0; i < 4; ++i) out[(16 * M + 4 * g + i) * BH_LR + col] = acc[e][i];
    }
  }
}

// ---- cell adjoints ----
// BPTT cell adjoint of one (row, unit) at step t: gates tg = (i, f, g, o), c = c_t, cp = c_{t-1} (0 at t = 0),
// dh = the step's dH, hrec = dz_{t+1} U^T.  Updates the carry dc, writes dz_t = z4 to the cell's words of the
// fp32 dz tile (zrow; a padding cell: the trash row) and returns the total h adjoint dht
template <int ACT>
__device__ __forceinline__ float bptt_cell(f32x4& z4, float& dc, const f32x4 tg, float c, float cp, float dh, float hrec,
                                           bool tok, float* zrow, float* trash) {
  const float ig = tg[0], fg = tg[1], gg = tg[2], og = tg[3];
  const float dht = dh + hrec;
  const float ca = act_f(ACT, c);
  const float dov = dht * ca;
  const float dct = dc + dht * og * act_dy(ACT, ca);
  dc = tok ? dct * fg : 0.f;
  z4[0] = dct * gg * ig * (1.f - ig);
  z4[1] = dct * cp * fg * (1.f - fg);
  z4[2] = dct * ig * act_dy(ACT, gg);
  z4[3] = dov * og * (1.f - og);
  float* zd = tok ? zrow : trash;
#pragma unroll
  for (int k = 0; k < 4; ++k) zd[k * BZ_KQ] = z4[k];
  return dht;
}

// tangent-reverse cell adjoint of one (row, unit): primal gates tg and their pre-activation tangents tz,
// c / cd = c_t / cdot_t, cp / cdp = those of t - 1.  The total adjoint of h_t is dh + *hrec (the step's dH and
// the cell's word of dz_{t+1} U^T); that of hdot_t is dhd + *hdrec with ZD, and dhd itself without (the
// single-stream kernel reads it whole, hdrec null).  Updates the carries acn / acdn and writes dz_t to the
// cell's words zt + zo of the dz tile; ZD: the tangent stream's own dzdot_t to zdt + zo as well.  (The sums
// are formed here, after the activation terms, and the addresses after the products: the statement order of
// the kernels this came from, which the packed-math pairing and with it the fused roundings follow)
template <int ACT, bool ZD>
__device__ __forceinline__ void tan_cell(float& acn, float& acdn, const f32x4 tg, const f32x4 tz, float c, float cd,
                                         float cp, float cdp, float dh, const float* hrec, float dhd, const float* hdrec,
                                         bool tok, float* zt, float* zdt, int zo, float* trash) {
  const float i_ = tg[0], f_ = tg[1], g_ = tg[2], o_ = tg[3];
  const float zdi = tz[0], zdf = tz[1], zdg = tz[2], zdo = tz[3];
  const float si = i_ * (1.f - i_), sf = f_ * (1.f - f_), so = o_ * (1.f - o_), sg = act_dy(ACT, g_);
  const float idot = si * zdi, fdot = sf * zdf, gdot = sg * zdg, odot = so * zdo;
  const float ca = act_f(ACT, c), d1 = act_dy(ACT, ca), d2 = act_d2y(ACT, ca);
  const float a_h = dh + *hrec;
  float a_hd = dhd;
  if constexpr (ZD) a_hd = dhd + *hdrec;
  const float a_od = a_hd * ca;
  const float a_o = a_h * ca + a_hd * d1 * cd;
  const float a_cd = acdn + a_hd * o_ * d1;
  const float a_c = acn + a_h * o_ * d1 + a_hd * (odot * d1 + o_ * d2 * cd);
  const float a_fd = a_cd * cp, a_id = a_cd * g_, a_gd = a_cd * i_;
  const float a_f = a_c * cp + a_cd * cdp;
  const float a_i = a_c * g_ + a_cd * gdot;
  const float a_g = a_c * i_ + a_cd * idot;
  acn = tok ? a_c * f_ + a_cd * fdot : 0.f;
  acdn = tok ? a_cd * f_ : 0.f;
  const float s2i = si * (1.f - 2.f * i_), s2f = sf * (1.f - 2.f * f_), s2o = so * (1.f - 2.f * o_);
  const float s2g = act_d2y(ACT, g_);
  float z4[4];
  z4[0] = a_i * si + a_id * s2i * zdi;
  z4[1] = a_f * sf + a_fd * s2f * zdf;
  z4[2] = a_g * sg + a_gd * s2g * zdg;
  z4[3] = a_o * so + a_od * s2o * zdo;
  float* zq = tok ? zt + zo : trash;
  if constexpr (ZD) {
    const float zd4[4] = {a_id * si, a_fd * sf, a_gd * sg, a_od * so};
    float* zdq = tok ? zdt + zo : trash;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      zq[k * BZ_KQ] = z4[k];
      zdq[k * BZ_KQ] = zd4[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) zq[k * BZ_KQ] = z4[k];
  }
}
// the tangent reverse's step loads of cell (half m, unit tile n) at step tt: gates, zdot, c_{tt-1}, cdot_{tt-1}
// and dH (HEAD: the product hdm * w[tt, unit], whose w is returned for a second factor).  The per-lane part of
// every address is one of tl, tcl, vp, hvo; the cell's slot and the step go into the uniform soffset, so no
// per-cell offset registers are hoisted (out-of-range lanes: voffset kOOB, which the range check drops
// whatever the soffset)
template <bool HEAD>
__device__ __forceinline__ float tan_step_load(f32x4& tg, f32x4& tz, float& tcp, float& tcdp, float& tdh, rsrc_t rt,
                                               rsrc_t rtt, rsrc_t rdh, rsrc_t rhw, int tl, int tcl, int vp, int hvo,
                                               float hdm, int m, int n, int tt, bool tok) {
  const int tp = tt > 0 ? tt - 1 : 0;
  const int sg = tt * FT_STEP * 4 + ftape_slot(m, n), sc = tp * FT_STEP * 4 + ftape_slot(m, n);
  const int sd = tt * FH * 4 + 16 * n;
  tg = ld4s(rt, tok ? tl : kOOB, sg);
  tz = ld4s(rtt, tok ? tl : kOOB, sg);
  tcp = ld1(rt, (tok && tt > 0) ? tcl : kOOB, sc);
  tcdp = ld1(rtt, (tok && tt > 0) ? tcl : kOOB, sc);
  float wv = 0.f;
  if constexpr (HEAD) {
    wv = ld1(rhw, tok ? hvo : kOOB, sd);
    tdh = hdm * wv;
  } else {
    tdh = ld1(rdh, tok ? vp : kOOB, sd);
  }
  return wv;
}
// HEAD: dH is the critic head's outer product f (x) w.  The factor of the lane's two rows
// (row0 + 16 m + 4 g + q; 0 past B, for an absent factor and without HEAD) and the head weight's descriptor
template <bool HEAD>
__device__ __forceinline__ void head_rows(float (&v)[2], const float* f, bool have, int row0, int B, int g, int q) {
  v[0] = v[1] = 0.f;
  if constexpr (HEAD) {
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int r = row0 + 16 * m + 4 * g + q;
      v[m] = (have && r < B) ? f[r] : 0.f;
    }
  }
}
template <bool HEAD>
__device__ __forceinline__ rsrc_t head_rsrc(const float* hw, int Tn) { return make_rsrc(hw, HEAD ? Tn * FH * 4 : 0); }

// ------------------------------------------------------------------------------------------
// BPTT with a role split and a row-half pipeline (8 waves, two per SIMD).
//
// A BPTT that runs the step's MFMA phase (dh_rec = dz_{t+1} U^T) and its VALU phase (the cell
// adjoints) back to back in the same four waves leaves the matrix pipe idle through every VALU phase:
// 400 MFMAs = 12.8 k cycles of pipe time per wave and step against ~24 k measured.  A single wave
// cannot overlap them (in-order issue; the scheduler keeps the cell math in clumps between MFMA
// runs), so here the roles go to different waves that share a SIMD:
//   * waves 0..3 (MFMA role): U^T fragments in AGPRs (the same 2 column tiles per wave as before)
//     and nothing else; A(m, t) = rows m of dh_rec(t) -> the dh tile;
//   * waves 4..7 (cell role): the cell state, tape loads and dZ stores of units 28 w' .. 28 w' + 27;
//     B(m, t) = the cell adjoints of rows m, which overwrite rows m of the dz tile with dz_t.
// The two 16-row halves of a tile are independent recurrences (the A operand of row r is
// dz_{t+1}[r]), so one role works on one half while the other role works on the other half:
//   P1(t): B(0, t) || A(1, t)      P2(t): B(1, t) || A(0, t - 1)
// with one barrier after each.  The hardware interleaves the two waves of a SIMD, so the cell math
// issues while the matrix pipe runs.  Register budget: the MFMA role ~230 (200 AGPRs of U^T), the
// cell role ~150, two waves per SIMD.  dZ rows of a half leave during the half-phase after the one
// that completed them (the tile rows are stable for exactly that phase).  The dz / dh tiles start at
// zero (dz_T = 0, dh_rec(T - 1) = 0), so the first P1 and the last P2 need no special case
// (A(0, -1) is computed into dh rows 0 and never read).
template <int ACT>
__global__ void __launch_bounds__(512, 1)
lstmf_bwdp_kernel(const float* __restrict__ dH, const float* __restrict__ tape, const float* __restrict__ U,
                  float* __restrict__ dZ, int B, int Tn) {
  extern __shared__ __attribute__((aligned(16))) float fsm[];
  float* zt = fsm;                  // dz tile [32][BZ_LR]: [q][u'] per row
  float* ht = zt + 32 * BZ_LR;      // dh_rec tile [32][BH_LR]
  float* trash = ht + 32 * BH_LR;   // [4 * BZ_KQ] written by padding cells, never read
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int w = wv & 3;             // wave index within the role
  const int q = lane & 3, g = lane >> 4, j4 = (lane & 15) >> 2, c16 = lane & 15;
  const int nrb = (B + 31) / 32;
  if (wv < 4) {
    // ---------------- MFMA role ----------------
    float ut[2][FH];
    rev_ut_load(ut, U, w, c16, g);
    for (int rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
      for (int i = tid; i < 32 * BZ_LR; i += 512) zt[i] = 0.f;  // dz_T = 0
      for (int i = tid; i < 32 * BH_LR; i += 512) ht[i] = 0.f;  // dh_rec(T - 1) = 0
      __syncthreads();
      for (int t = Tn - 1; t >= 0; --t) {
        rev_half_a<1, 4>(zt, ht, ut, w, c16, g);  // P1(t): A(1, t)
        lds_barrier();
        rev_half_a<0, 4>(zt, ht, ut, w, c16, g);  // P2(t): A(0, t - 1)
        lds_barrier();
      }
      __syncthreads();
    }
  } else {
    // ---------------- cell role ----------------
    const int ct = tid - 256;
    const int ub = FUW * w + j4;
    const int hr = (4 * g + q) * BH_LR + ub, zw = (4 * g + q) * BZ_LR + ub;
    const RevStore st(ct, Tn);  // threads 0..199 of the role
    const int tl = ftape_lane(w, lane), tcl = ftape_cell(w, lane);
    for (int rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
      const int row0 = rb * 32;
      const rsrc_t rdh = ftile_rsrc(dH, row0, B, Tn, FH), rt = ftape_rsrc(tape, rb, nrb, Tn);
      const rsrc_t rz = ftile_rsrc(dZ, row0, B, Tn, FG);
      const int nr = min(32, B - row0);
      int vp1[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) vp1[m] = ((16 * m + 4 * g + q) * Tn * FH + ub) * 4;
      float dc[2][FNT], tc[2][FNT];
      f32x4 tg[2][FNT];
      float tcp[2][FNT], tdh[2][FNT];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < FNT; ++n) {
          const bool tok = unit_ok(w, n);
          const int T1 = Tn - 1;
          dc[m][n] = 0.f;
          tc[m][n] = ld1(rt, tok ? tcl + T1 * FT_STEP * 4 + ftape_slot(m, n) : kOOB, 0);  // c_{T-1}
          bwdf_tape_load(tg[m][n], tcp[m][n], tdh[m][n], rt, rdh, tl + T1 * FT_STEP * 4 + ftape_slot(m, n),
                         tcl + (T1 - 1) * FT_STEP * 4 + ftape_slot(m, n), vp1[m] + T1 * FH * 4 + 16 * n, tok, T1 > 0);
        }
      for (int i = tid; i < 32 * BZ_LR; i += 512) zt[i] = 0.f;
      for (int i = tid; i < 32 * BH_LR; i += 512) ht[i] = 0.f;
      __syncthreads();
      // cell adjoints of row half M at step t; each cell then issues step t - 1's tape loads
      auto half_b = [&](auto M_, int t) {
        constexpr int m = decltype(M_)::value;
#pragma unroll
        for (int n = 0; n < FNT; ++n) {
          const bool tok = unit_ok(w, n);
          f32x4 z4;
          bptt_cell<ACT>(z4, dc[m][n], tg[m][n], tc[m][n], tcp[m][n], tdh[m][n], ht[hr + 16 * m * BH_LR + 4 * n], tok,
                         zt + zw + 16 * m * BZ_LR + 4 * n, trash);
          tc[m][n] = tcp[m][n];  // c_{t-1} is the next step's c
          const int tp = t > 0 ? t - 1 : 0;
          bwdf_tape_load(tg[m][n], tcp[m][n], tdh[m][n], rt, rdh, tl + tp * FT_STEP * 4 + ftape_slot(m, n),
                         tcl + (tp - 1) * FT_STEP * 4 + ftape_slot(m, n), vp1[m] + tp * FH * 4 + 16 * n,
                         tok && t > 0, tp > 0);
        }
      };
      for (int t = Tn - 1; t >= 0; --t) {
        if (t < Tn - 1) st.half<1, false>(zt, rz, Tn, t + 1, nr);  // rows 16..31 of dz_{t+1}: stable until P2(t)
        half_b(I0{}, t);                                           // P1(t): B(0, t)
        lds_barrier();
        st.half<0, false>(zt, rz, Tn, t, nr);                      // rows 0..15 of dz_t: stable until P1(t - 1)
        half_b(I1{}, t);                                           // P2(t): B(1, t)
        lds_barrier();
      }
      st.half<1, false>(zt, rz, Tn, 0, nr);
      __syncthreads();  // (the tiles are re-zeroed for the next row block)
    }
  }
}

// ==========================================================================================
// tangent reverse (fp32): (dZ, dZdot) of the reverse-over-tangent pass (ops/reference.py
// lstm_seq_tbwd) from the primal and tangent tapes of lstmf_fwd<TAPE> / lstmf_fwd<TAN>
// ==========================================================================================
// ------------------------------------------------------------------------------------------
// tangent reverse with the role split of lstmf_bwdp_kernel: 32-row tiles whose 16-row halves are
// pipelined (P1(t): cells of rows 0-15 || MFMAs of rows 16-31; P2(t): cells of rows 16-31 ||
// MFMAs of rows 0-15 of the previous step), MFMA waves 0..3 (U^T in VGPRs, both adjoint streams:
// 400 MFMAs per half-phase) and cell waves 4..7.  The cell waves carry 4 values per cell for both
// halves (c, cdot and the two adjoint carries) and ONE set of step loads (gates, zdot, c_{t-1},
// cdot_{t-1}, dH, dHd: 12 per cell): the set for the other half is issued right after a half's
// cells, and lands while the MFMA waves finish the half-phase.
// Cells whose temporaries share one schedule region of the cell role, in both tangent kernels: 2
// (lstmf_tbwdp_kernel: 13.80 -> 13.45 ms per call at B = 262 144; one cell at a time was the round-4
// schedule, seven 13.56 ms: profiles/r05_tbwd/README.md.  lstmf_tbwd1_kernel: 4 and 7 measured neutral,
// docs/PERF.md)
constexpr int kTanCellGroup = 2;
template <int ACT, bool HEAD = false>
__global__ void __launch_bounds__(512, 1)
lstmf_tbwdp_kernel(const float* __restrict__ dH, const float* __restrict__ dHd, const float* __restrict__ tape,
                   const float* __restrict__ ttape, const float* __restrict__ U, float* __restrict__ dZ,
                   float* __restrict__ dZd, int B, int Tn, const float* __restrict__ hd, const float* __restrict__ hdd,
                   const float* __restrict__ hw) {
  extern __shared__ __attribute__((aligned(16))) float fsm[];
  float* zt = fsm;                   // dz tile     [32][BZ_LR]
  float* zdt = zt + 32 * BZ_LR;      // dzdot tile  [32][BZ_LR]
  float* ht = zdt + 32 * BZ_LR;      // dz U^T      [32][BH_LR]
  float* hdt = ht + 32 * BH_LR;      // dzdot U^T   [32][BH_LR]
  float* trash = hdt + 32 * BH_LR;   // [4 * BZ_KQ] padding-cell writes
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int w = wv & 3;
  const int q = lane & 3, g = lane >> 4, j4 = (lane & 15) >> 2, c16 = lane & 15;
  const int nrb = (B + 31) / 32;
  if (wv < 4) {
    // ---------------- MFMA role ----------------
    float ut[2][FH];
    rev_ut_load(ut, U, w, c16, g);
    // rows of half M of (dz, dzdot) U^T, one adjoint stream after the other (8 accumulator
    // registers live: U^T takes 200 of the role's 256 VGPRs)
    auto half_a = [&](auto M_) {
      constexpr int M = decltype(M_)::value;
      rev_half_a<M, 2>(zt, ht, ut, w, c16, g);
      rev_half_a<M, 2>(zdt, hdt, ut, w, c16, g);
    };
    // the dz / dzdot stores ride on the MFMA role (they were 6 % of the cell role's time, which
    // sets the half-phase length)
    const RevStore st(tid, Tn);
    for (int rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
      const int row0 = rb * 32;
      const rsrc_t rz = ftile_rsrc(dZ, row0, B, Tn, FG), rzd = ftile_rsrc(dZd, row0, B, Tn, FG);
      const int nr = min(32, B - row0);
      auto store_half = [&](auto M_, int ts) {
        constexpr int M = decltype(M_)::value;
        st.half<M, true>(zt, rz, Tn, ts, nr);
        st.half<M, true>(zdt, rzd, Tn, ts, nr);
      };
      for (int i = tid; i < 2 * 32 * (BZ_LR + BH_LR); i += 512) zt[i] = 0.f;  // all four tiles
      __syncthreads();
      for (int t = Tn - 1; t >= 0; --t) {
        if (t < Tn - 1) store_half(I1{}, t + 1);  // rows 16..31 of dz_{t+1}: stable during P1(t)
        half_a(I1{});
        lds_barrier();
        store_half(I0{}, t);                      // rows 0..15 of dz_t: stable during P2(t)
        half_a(I0{});
        lds_barrier();
      }
      store_half(I1{}, 0);
      __syncthreads();
    }
  } else {
    // ---------------- cell role ----------------
    // (the c_{T-1} / cdot_{T-1} prologue stays written out: as a helper, alone on this kernel, it changed 49 of the
    // 135 lstmf_tbwd arrays of the A/B against the parent build in their last bits,
    // profiles/lstmf_rev_shared/single_helper.txt)
    const int ub = FUW * w + j4;
    const int hr = (4 * g + q) * BH_LR + ub, zw = (4 * g + q) * BZ_LR + ub;
    const int tl = ftape_lane(w, lane), tcl = ftape_cell(w, lane);
    for (int rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
      const int row0 = rb * 32;
      const rsrc_t rdh = ftile_rsrc(dH, row0, B, Tn, FH), rdhd = ftile_rsrc(dHd, row0, B, Tn, FH);
      const rsrc_t rt = ftape_rsrc(tape, rb, nrb, Tn), rtt = ftape_rsrc(ttape, rb, nrb, Tn);
      int vp1[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) vp1[m] = ((16 * m + 4 * g + q) * Tn * FH + ub) * 4;
      // HEAD: dH = hd (x) w, dHd = hdd (x) w generated per cell (a null factor: that adjoint is zero)
      float hdv[2], hddv[2];
      head_rows<HEAD>(hdv, hd, hd != nullptr, row0, B, g, q);
      head_rows<HEAD>(hddv, hdd, hdd != nullptr, row0, B, g, q);
      const rsrc_t rhw = head_rsrc<HEAD>(hw, Tn);
      const int hvo = ub * 4;
      float tc[2][FNT], tcd[2][FNT], acn[2][FNT], acdn[2][FNT];
      f32x4 tg[FNT], tz[FNT];
      float tcp[FNT], tcdp[FNT], tdh[FNT], tdhd[FNT];
      // the step loads of half M at step tt (one register set, reused by the two halves in turn).
      // The per-lane part of every address is one of four VGPRs (tl, tcl, vp1[m]); the cell's slot
      // and the step go into the uniform soffset, so no per-cell offset registers are hoisted
      // (out-of-range lanes: voffset kOOB, which the range check drops whatever the soffset)
      auto load_half = [&](auto M_, int tt, bool on) {
        constexpr int m = decltype(M_)::value;
#pragma unroll
        for (int n = 0; n < FNT; ++n) {
          const bool tok = on && unit_ok(w, n);
          const float wn = tan_step_load<HEAD>(tg[n], tz[n], tcp[n], tcdp[n], tdh[n], rt, rtt, rdh, rhw, tl, tcl, vp1[m],
                                               hvo, hdv[m], m, n, tt, tok);
          if constexpr (HEAD) tdhd[n] = hddv[m] * wn;
          else tdhd[n] = ld1(rdhd, tok ? vp1[m] : kOOB, tt * FH * 4 + 16 * n);
        }
      };
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < FNT; ++n) {
          const bool tok = unit_ok(w, n);
          const int oc = tcl + (Tn - 1) * FT_STEP * 4 + ftape_slot(m, n);
          acn[m][n] = 0.f;
          acdn[m][n] = 0.f;
          tc[m][n] = ld1(rt, tok ? oc : kOOB, 0);
          tcd[m][n] = ld1(rtt, tok ? oc : kOOB, 0);
        }
      load_half(I0{}, Tn - 1, true);
      for (int i = tid; i < 2 * 32 * (BZ_LR + BH_LR); i += 512) zt[i] = 0.f;
      __syncthreads();
      auto half_b = [&](auto M_) {
        constexpr int m = decltype(M_)::value;
#pragma unroll
        for (int n = 0; n < FNT; ++n) {
          const int hi = hr + 16 * m * BH_LR + 4 * n, zo = zw + 16 * m * BZ_LR + 4 * n;
          tan_cell<ACT, true>(acn[m][n], acdn[m][n], tg[n], tz[n], tc[m][n], tcd[m][n], tcp[n], tcdp[n], tdh[n], ht + hi,
                              tdhd[n], hdt + hi, unit_ok(w, n), zt, zdt, zo, trash);
          tc[m][n] = tcp[n];
          tcd[m][n] = tcdp[n];
          if ((n + 1) % kTanCellGroup == 0 || n == FNT - 1) __builtin_amdgcn_sched_barrier(0);
        }
      };
      for (int t = Tn - 1; t >= 0; --t) {
        half_b(I0{});                             // P1(t): B(0, t)
        __builtin_amdgcn_sched_barrier(0);        //   (the load set is free only after the cells)
        load_half(I1{}, t, true);                 //   then half 1's loads for P2(t)
        lds_barrier();
        half_b(I1{});                             // P2(t): B(1, t)
        __builtin_amdgcn_sched_barrier(0);
        load_half(I0{}, t > 0 ? t - 1 : 0, t > 0);  //   then half 0's loads for P1(t - 1)
        lds_barrier();
      }
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------------------------------
// single-stream tangent reverse: lstmf_tbwd1_kernel
// ------------------------------------------------------------------------------------------
// The tangent system is the linearisation of the primal one, so the adjoint of every tangent quantity
// (a_hd, a_cd, dzd) depends on no tangent value: it is the plain BPTT of the tangent seed dHd.  When that
// BPTT has already run (the gradient penalty: the BPTT on x_hat seeded with ones, then the tangent reverse
// seeded with ones), its per-step total h adjoint aH (lstmf_bwds_kernel<.., AHD>) is this kernel's a_hd and
// its dZ is the dZd operand of the weight gradient: here only the primal adjoint stream runs
// (ops/reference.py lstm_seq_tbwd_ahd).  a_cd follows from a_hd by the elementwise carry
// a_cd = acd_n + a_hd o d1, acd_n = a_cd f.  lstmf_tbwdp_kernel's layout minus the second stream: the MFMA
// role issues 200 exact-fp32 MFMAs per half-phase (dz U^T only) and stores dZ, the cell role carries three
// values per cell and half (c, cdot via the tapes, the two carries) and one set of step loads (gates, zdot,
// c_{t-1}, cdot_{t-1}, dH, aH).  dH / the head factor hd may be null (no primal seed).
template <int ACT, bool HEAD = false>
__global__ void __launch_bounds__(512, 1)
lstmf_tbwd1_kernel(const float* __restrict__ dH, const float* __restrict__ aH, const float* __restrict__ tape,
                   const float* __restrict__ ttape, const float* __restrict__ U, float* __restrict__ dZ, int B, int Tn,
                   const float* __restrict__ hd, const float* __restrict__ hw) {
  extern __shared__ __attribute__((aligned(16))) float fsm[];
  float* zt = fsm;                   // dz tile  [32][BZ_LR]
  float* ht = zt + 32 * BZ_LR;       // dz U^T   [32][BH_LR]
  float* trash = ht + 32 * BH_LR;    // [4 * BZ_KQ] padding-cell writes
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int w = wv & 3;
  const int q = lane & 3, g = lane >> 4, j4 = (lane & 15) >> 2, c16 = lane & 15;
  const int nrb = (B + 31) / 32;
  if (wv < 4) {
    // ---------------- MFMA role ----------------
    float ut[2][FH];
    rev_ut_load(ut, U, w, c16, g);
    const RevStore st(tid, Tn);  // the dz stores ride on the MFMA role
    for (int rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
      const int row0 = rb * 32;
      const rsrc_t rz = ftile_rsrc(dZ, row0, B, Tn, FG);
      const int nr = min(32, B - row0);
      for (int i = tid; i < 32 * (BZ_LR + BH_LR); i += 512) zt[i] = 0.f;  // both tiles
      __syncthreads();
      for (int t = Tn - 1; t >= 0; --t) {
        if (t < Tn - 1) st.half<1, true>(zt, rz, Tn, t + 1, nr);  // rows 16..31 of dz_{t+1}: stable during P1(t)
        rev_half_a<1, 2>(zt, ht, ut, w, c16, g);
        lds_barrier();
        st.half<0, true>(zt, rz, Tn, t, nr);                      // rows 0..15 of dz_t: stable during P2(t)
        rev_half_a<0, 2>(zt, ht, ut, w, c16, g);
        lds_barrier();
      }
      st.half<1, true>(zt, rz, Tn, 0, nr);
      __syncthreads();
    }
  } else {
    // ---------------- cell role ----------------
    // (written out here: the cell adjoint -- tan_cell<ACT, false> alone on this kernel changed 15 of the 108
    // lstmf_tbwd1 arrays of the A/B against the parent build in their last bits -- and the prologue, 56 of 108:
    // profiles/lstmf_rev_shared/single_helper.txt)
    const int ub = FUW * w + j4;
    const int hr = (4 * g + q) * BH_LR + ub, zw = (4 * g + q) * BZ_LR + ub;
    const int tl = ftape_lane(w, lane), tcl = ftape_cell(w, lane);
    for (int rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
      const int row0 = rb * 32;
      const rsrc_t rdh = ftile_rsrc(dH, row0, B, Tn, FH), rah = ftile_rsrc(aH, row0, B, Tn, FH);
      const rsrc_t rt = ftape_rsrc(tape, rb, nrb, Tn), rtt = ftape_rsrc(ttape, rb, nrb, Tn);
      int vp1[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) vp1[m] = ((16 * m + 4 * g + q) * Tn * FH + ub) * 4;
      // HEAD: dH = hd (x) w generated per cell (a null factor: the primal seed is zero)
      float hdv[2];
      head_rows<HEAD>(hdv, hd, hd != nullptr, row0, B, g, q);
      const rsrc_t rhw = head_rsrc<HEAD>(hw, Tn);
      const int hvo = ub * 4;
      float tc[2][FNT], tcd[2][FNT], acn[2][FNT], acdn[2][FNT];
      f32x4 tg[FNT], tz[FNT];
      float tcp[FNT], tcdp[FNT], tdh[FNT], tah[FNT];
      // the step loads of (half M, cell n) at step tt (one register set, reused by the two halves in turn).
      // The per-lane part of every address is one of four VGPRs (tl, tcl, vp1[m]); the cell's slot
      // and the step go into the uniform soffset, so no per-cell offset registers are hoisted
      // (out-of-range lanes: voffset kOOB, which the range check drops whatever the soffset)
      auto load_cell = [&](auto M_, int n, int tt, bool on) {
        constexpr int m = decltype(M_)::value;
        const bool tok = on && unit_ok(w, n);
        tan_step_load<HEAD>(tg[n], tz[n], tcp[n], tcdp[n], tdh[n], rt, rtt, rdh, rhw, tl, tcl, vp1[m], hvo, hdv[m], m, n, tt,
                            tok);
        tah[n] = ld1(rah, tok ? vp1[m] : kOOB, tt * FH * 4 + 16 * n);
      };
      auto load_half = [&](auto M_, int tt, bool on) {
#pragma unroll
        for (int n = 0; n < FNT; ++n) load_cell(M_, n, tt, on);
      };
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < FNT; ++n) {
          const bool tok = unit_ok(w, n);
          const int oc = tcl + (Tn - 1) * FT_STEP * 4 + ftape_slot(m, n);
          acn[m][n] = 0.f;
          acdn[m][n] = 0.f;
          tc[m][n] = ld1(rt, tok ? oc : kOOB, 0);
          tcd[m][n] = ld1(rtt, tok ? oc : kOOB, 0);
        }
      load_half(I0{}, Tn - 1, true);
      for (int i = tid; i < 32 * (BZ_LR + BH_LR); i += 512) zt[i] = 0.f;
      __syncthreads();
      // cells of half M.  Each cell issues the loads of the set's next use (half MN at step tn) right after its
      // own math, as lstmf_bwds_kernel's cells do: with half the matrix work the cell role waits on its loads,
      // not on the MFMA role (all seven after the last cell, lstmf_tbwdp_kernel's order, was measured +6 % per
      // call; a second register set for the 16-byte loads spills: docs/PERF.md)
      auto half_b = [&](auto M_, auto MN_, int tn, bool non) {
        constexpr int m = decltype(M_)::value;
#pragma unroll
        for (int n = 0; n < FNT; ++n) {
          const bool tok = unit_ok(w, n);
          const float i_ = tg[n][0], f_ = tg[n][1], g_ = tg[n][2], o_ = tg[n][3];
          const float zdi = tz[n][0], zdf = tz[n][1], zdg = tz[n][2], zdo = tz[n][3];
          const float c = tc[m][n], cd = tcd[m][n], cp = tcp[n], cdp = tcdp[n];
          const float si = i_ * (1.f - i_), sf = f_ * (1.f - f_), so = o_ * (1.f - o_), sg = act_dy(ACT, g_);
          const float idot = si * zdi, fdot = sf * zdf, gdot = sg * zdg, odot = so * zdo;
          const float ca = act_f(ACT, c), d1 = act_dy(ACT, ca), d2 = act_d2y(ACT, ca);
          const float a_h = tdh[n] + ht[hr + 16 * m * BH_LR + 4 * n], a_hd = tah[n];
          const float a_od = a_hd * ca;
          const float a_o = a_h * ca + a_hd * d1 * cd;
          const float a_cd = acdn[m][n] + a_hd * o_ * d1;
          const float a_c = acn[m][n] + a_h * o_ * d1 + a_hd * (odot * d1 + o_ * d2 * cd);
          const float a_fd = a_cd * cp, a_id = a_cd * g_, a_gd = a_cd * i_;
          const float a_f = a_c * cp + a_cd * cdp;
          const float a_i = a_c * g_ + a_cd * gdot;
          const float a_g = a_c * i_ + a_cd * idot;
          acn[m][n] = tok ? a_c * f_ + a_cd * fdot : 0.f;
          acdn[m][n] = tok ? a_cd * f_ : 0.f;
          const float s2i = si * (1.f - 2.f * i_), s2f = sf * (1.f - 2.f * f_), s2o = so * (1.f - 2.f * o_);
          const float s2g = act_d2y(ACT, g_);
          float z4[4];
          z4[0] = a_i * si + a_id * s2i * zdi;
          z4[1] = a_f * sf + a_fd * s2f * zdf;
          z4[2] = a_g * sg + a_gd * s2g * zdg;
          z4[3] = a_o * so + a_od * s2o * zdo;
          float* zp = tok ? zt + zw + 16 * m * BZ_LR + 4 * n : trash;
#pragma unroll
          for (int k = 0; k < 4; ++k) zp[k * BZ_KQ] = z4[k];
          tc[m][n] = cp;
          tcd[m][n] = cdp;
          load_cell(MN_, n, tn, non);
          if ((n + 1) % kTanCellGroup == 0 || n == FNT - 1) __builtin_amdgcn_sched_barrier(0);
        }
      };
      for (int t = Tn - 1; t >= 0; --t) {
        half_b(I0{}, I1{}, t, true);                        // P1(t): B(0, t), then half 1's loads for P2(t)
        lds_barrier();
        half_b(I1{}, I0{}, t > 0 ? t - 1 : 0, t > 0);       // P2(t): B(1, t), then half 0's loads for P1(t - 1)
        lds_barrier();
      }
      __syncthreads();
    }
  }
}

// ==========================================================================================
// forward / tangent forward with the recurrent product on the bf16 pipe (K <= 36 layers)
// ==========================================================================================
// lstmf_fwd_kernel spends 25 of its 33 k-steps per tile on h_{t-1} U (K = 32: 800 of 1056 MFMA cycles
// per tile and row half on v_mfma_f32_16x16x4_f32).  Here h_{t-1} U runs as the exact three-term split
// (h = h_h + h_m + h_l, U = U_h + U_m + U_l by truncation, six products lh + hl + mm + mh + hm + hh on
// v_mfma_f32_16x16x32_bf16, dropped terms <= 2^-24 of each product) over k = 0..95 and exactly in fp32
// for k = 96..99 (one 16x16x4 k-step): 3 x 6 x 16 + 32 = 320 instead of 800 cycles per tile and row
// half.  The split products chain into the exact-fp32 x W accumulator.  U's planes (3 k-steps x 7 tiles x 3 planes, 252 registers) are pinned in AGPRs; h_{t-1} lives
// in LDS as three bf16 planes [32 rows][104] (row stride: conflict-free ds_read_b128) plus an fp32
// tail [32][4]; the cell update writes its h (or hdot) straight into them.  Everything else -- the
// gate-interleaved tiles, the quad transpose, the tapes, x W on the exact fp32 MFMA -- is
// lstmf_fwd_kernel's.
// Plane row strides for the 16x16x32 A-fragment ds_read_b128 (lane l: row l & 15, k-group l >> 4, i.e.
// dword S (l & 15) + 4 (l >> 4)): conflict-free over the CDNA4 b128 lane groups {0-3,12-15,20-27},
// {4-11,16-19,28-31} (+32) only for S = 56, 72 (mod 64 multiples) / 216, 232, 248 dwords; the r03 strides
// (52 / 212 dwords) were conflict-free for contiguous 16-lane groups only and 2-way on the real ones
// (bwds: SQ_LDS_BANK_CONFLICT 1.56x its LDS-active cycles, profiles/r03_bwds/pmc_bptt_B262144.txt)
constexpr int FS_HR = 112;                                // h plane row stride (bf16 elements): 56 dwords
constexpr int FS_HPL = 32 * FS_HR * 2;                    // bytes per h plane (32 rows)
constexpr int FS_HB = 3 * FS_HPL + 32 * 4 * 4;            // one h buffer: 3 planes + fp32 tail [32][4]

template <int ACT, int KX, bool TAPE, bool TAN>
__global__ void __launch_bounds__(256, 1)
lstmf_fwds_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                  const float* __restrict__ U, const float* __restrict__ ptape, float* __restrict__ hs,
                  float* __restrict__ tape, int B, int Tn) {
  using GX = FGeo<KX>;
  static_assert(GX::KS <= 12, "split forward: K <= 48 (W^T in registers)");
  constexpr int NW = GX::KS;
  extern __shared__ __attribute__((aligned(16))) float fsm[];
  float* xb = fsm;                                                  // [2][32 * LRX] fp32, K-permuted
  float* trash = xb + 2 * 32 * GX::LR;                              // [4] padding / out-of-range writes
  lds_char* trashc = (lds_char*)trash;
  lds_char* hb = (lds_char*)(trash + 4);                            // [2][FS_HB] h planes + tail
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = lane & 3, g = lane >> 4, j4 = (lane & 15) >> 2;
  const int ub = FUW * w + j4;
  const int nrb = (B + 31) / 32;

  for (int i = tid; i < 2 * 32 * GX::LR; i += 256) xb[i] = 0.f;

  constexpr float GSC = ACT == ACT_TANH ? -2.f * kLog2e : ACT == ACT_SIGMOID ? -kLog2e : 1.f;
  const float sc = TAN ? 1.f : (q == 2 ? GSC : -kLog2e);
  // B operands.  16x16x32: lane l holds B[k = 32 ks + 8 (l >> 4) + j][col l & 15] (j < 8); the fp32
  // tail 16x16x4: B[k = 96 + (l >> 4)][col]; x W (16x16x4): B[k = 4 ks + (l >> 4)][col]
  bf16x8 up[3][FNT][3];
  float ut[FNT], wf[NW][FNT], bq[FNT];
#pragma unroll
  for (int n = 0; n < FNT; ++n) {
    const int u = ub + 4 * n;
    const bool ok = u < FH;
    const int cl = q * FH + (ok ? u : FH - 1);
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) {
      uint32_t hh[8], mm[8], ll[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 32 * ks + 8 * g + j;  // < 96
        const float v = ok ? U[k * FG + cl] * sc : 0.f;
        const uint32_t h = trunc_hi(v);
        const float r1 = v - __builtin_bit_cast(float, h);
        const uint32_t m = trunc_hi(r1);
        const float r2 = r1 - __builtin_bit_cast(float, m);
        hh[j] = h; mm[j] = m; ll[j] = __builtin_bit_cast(uint32_t, r2);
      }
      uint4 ph, pm, pl;
      ph.x = __builtin_amdgcn_perm(hh[1], hh[0], 0x07060302u); ph.y = __builtin_amdgcn_perm(hh[3], hh[2], 0x07060302u);
      ph.z = __builtin_amdgcn_perm(hh[5], hh[4], 0x07060302u); ph.w = __builtin_amdgcn_perm(hh[7], hh[6], 0x07060302u);
      pm.x = __builtin_amdgcn_perm(mm[1], mm[0], 0x07060302u); pm.y = __builtin_amdgcn_perm(mm[3], mm[2], 0x07060302u);
      pm.z = __builtin_amdgcn_perm(mm[5], mm[4], 0x07060302u); pm.w = __builtin_amdgcn_perm(mm[7], mm[6], 0x07060302u);
      pl.x = __builtin_amdgcn_perm(ll[1], ll[0], 0x07060302u); pl.y = __builtin_amdgcn_perm(ll[3], ll[2], 0x07060302u);
      pl.z = __builtin_amdgcn_perm(ll[5], ll[4], 0x07060302u); pl.w = __builtin_amdgcn_perm(ll[7], ll[6], 0x07060302u);
      up[ks][n][0] = __builtin_bit_cast(bf16x8, ph);
      up[ks][n][1] = __builtin_bit_cast(bf16x8, pm);
      up[ks][n][2] = __builtin_bit_cast(bf16x8, pl);
#pragma unroll
      for (int p = 0; p < 3; ++p) asm volatile("" : "+a"(up[ks][n][p]));
    }
    ut[n] = ok ? U[(96 + g) * FG + cl] * sc : 0.f;
#pragma unroll
    for (int ks = 0; ks < NW; ++ks) {
      const int k = 4 * ks + g;
      const float v = W[min(k, KX - 1) * FG + cl];
      wf[ks][n] = (ok && k < KX) ? v * sc : 0.f;
    }
    const float bv = bias ? bias[cl] : 0.f;
    bq[n] = (!TAN && ok) ? bv * sc : 0.f;
  }
  const bool glin = !TAN && ACT == ACT_LINEAR && q == 2;
  const float am = (ACT == ACT_TANH && q == 2) ? 2.f : 1.f, bm = (ACT == ACT_TANH && q == 2) ? -1.f : 0.f;
  const int ax = (lane & 15) * GX::LR + g * GX::KQ;
  // this lane's h fragments: plane row (lane & 15) (+ 16 m), k = 32 ks + 8 g; tail row, k = 96 + g
  const int ahp = ((lane & 15) * FS_HR + 8 * g) * 2, aht = 3 * FS_HPL + ((lane & 15) * 4 + g) * 4;

  for (int rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int row0 = rb * 32;
    const rsrc_t rx = ftile_rsrc(x, row0, B, Tn, KX);
    const rsrc_t rh = ftile_rsrc(hs, row0, B, Tn, FH);
    const rsrc_t rt = ftape_rsrc(TAPE ? tape : nullptr, rb, nrb, Tn);
    const rsrc_t rp = ftape_rsrc(TAN ? ptape : nullptr, rb, nrb, Tn);
    int vp1[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) vp1[m] = ((16 * m + 4 * g + q) * Tn * FH + ub) * 4;
    const int tl = ftape_lane(w, lane), tcl = ftape_cell(w, lane);
    float cprev[TAN ? 2 : 1][FNT];
    if constexpr (TAN) {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < FNT; ++n) cprev[m][n] = 0.f;
    }
    float cst[2][FNT];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < FNT; ++n) cst[m][n] = 0.f;
    FXPart<KX> xp;
    xp.set(Tn, tid);
    xp.load(rx, Tn, 0, true);
    // h_{-1} = 0: buffer 0 planes + tail
    for (int i = tid; i < FS_HB / 16; i += 256)
      reinterpret_cast<__attribute__((address_space(3))) u32x4_t*>(hb)[i] = u32x4_t{0, 0, 0, 0};
    xp.to_lds(xb, trash);
    __syncthreads();
    for (int t = 0; t < Tn; ++t) {
      const float* xcur = xb + (t & 1) * 32 * GX::LR;
      const lds_char* hcur = hb + (t & 1) * FS_HB;
      lds_char* hnext = hb + ((t + 1) & 1) * FS_HB;
      xp.load(rx, Tn, t + 1, t + 1 < Tn);
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        f32x4 pg[TAN ? FNT : 1];
        float pc[TAN ? FNT : 1];
        const int p1 = vp1[m] + t * FH * 4, tb = t * FT_STEP * 4;
        if constexpr (TAN) {
#pragma unroll
          for (int n = 0; n < FNT; ++n) {
            const bool tok = !(w == 3 && n >= 4);
            pg[n] = ld4(rp, tok ? tl + tb + ftape_slot(m, n) : kOOB);
            pc[n] = ld1(rp, tok ? tcl + tb + ftape_slot(m, n) : kOOB, 0);
          }
        }
        f32x4 acc[FNT];
#pragma unroll
        for (int n = 0; n < FNT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
        // ---- z = x_t W (exact fp32) ----
#pragma unroll
        for (int j = 0; j < GX::NJ; ++j) {
          const f32x4 a4 = *reinterpret_cast<const f32x4*>(xcur + ax + 16 * m * GX::LR + 4 * j);
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) {
            const int ks = 4 * j + s4;
            if (ks >= GX::KS) break;
#pragma unroll
            for (int n = 0; n < FNT; ++n) acc[n] = mma4(a4[s4], wf[ks][n], acc[n]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        // ---- + h_{t-1} U: the split k < 96 and the exact fp32 tail, chained into acc (20 accumulation
        // steps per element: the MFMA C-addition rounding stays at the fp32 noise level here) ----
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) {
          const lds_char* ar = hcur + ahp + 16 * m * FS_HR * 2 + 64 * ks;
          const bf16x8 a[3] = {*reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>(ar),
                               *reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>(ar + FS_HPL),
                               *reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>(ar + 2 * FS_HPL)};
#pragma unroll
          for (int n = 0; n < FNT; ++n) acc[n] = mma_split6(a, up[ks][n], acc[n]);
          __builtin_amdgcn_sched_barrier(0);
        }
        {
          const float at = *reinterpret_cast<const __attribute__((address_space(3))) float*>(hcur + aht + 16 * m * 16);
#pragma unroll
          for (int n = 0; n < FNT; ++n) acc[n] = mma4(at, ut[n], acc[n]);
        }
        // ---- gate math, cell update, stores (row 16 m + 4 g + q, unit ub + 4 n after the transpose) ----
#pragma unroll
        for (int n = 0; n < FNT; ++n) {
          const bool tok = !(w == 3 && n >= 4);  // wave 3's tiles 4..6 are padding units 100..111
          const int v1 = tok ? p1 + 16 * n : kOOB;
          const f32x4 zs = acc[n];
          float hv;
          if constexpr (!TAN) {
            float y[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float s_ = zs[i] + bq[n];
              const float e = am * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(s_)) + bm;
              y[i] = glin ? s_ : e;
            }
            quad_transpose(y, q);
            const float cn = y[1] * cst[m][n] + y[0] * y[2];
            float ca;
            if constexpr (ACT == ACT_TANH) ca = 2.f * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(GSC * cn)) - 1.f;
            else if constexpr (ACT == ACT_SIGMOID) ca = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(GSC * cn));
            else ca = cn;
            hv = tok ? y[3] * ca : 0.f;
            cst[m][n] = cn;
            if constexpr (TAPE) {
              st4(f32x4{y[0], y[1], y[2], y[3]}, rt, tok ? tl + tb + ftape_slot(m, n) : kOOB);
              st1(cn, rt, tok ? tcl + tb + ftape_slot(m, n) : kOOB, 0);
            }
          } else {
            float zd[4] = {zs[0], zs[1], zs[2], zs[3]};
            quad_transpose(zd, q);
            const f32x4 y = pg[n];
            const float idot = y[0] * (1.f - y[0]) * zd[0], fdot = y[1] * (1.f - y[1]) * zd[1];
            const float gdot = act_dy(ACT, y[2]) * zd[2], odot = y[3] * (1.f - y[3]) * zd[3];
            const float c = pc[n];
            float cdn = fdot * cprev[m][n] + y[1] * cst[m][n] + idot * y[2] + y[0] * gdot;
            const float ca = act_f(ACT, c);
            float hd = odot * ca + y[3] * act_dy(ACT, ca) * cdn;
            if (!tok) { cdn = 0.f; hd = 0.f; }
            cst[m][n] = cdn;
            cprev[m][n] = c;
            hv = hd;
            st4(f32x4{zd[0], zd[1], zd[2], zd[3]}, rt, tok ? tl + tb + ftape_slot(m, n) : kOOB);
            st1(cdn, rt, tok ? tcl + tb + ftape_slot(m, n) : kOOB, 0);
          }
          // h (or hdot) of (row 16 m + 4 g + q, unit u) into the next step's planes / tail; units
          // >= 100 (wave 3's padding tiles) go to the trash word
          {
            const int u = ub + 4 * n, row = 16 * m + 4 * g + q;
            const uint32_t h1 = trunc_hi(hv);
            const float r1 = hv - __builtin_bit_cast(float, h1);
            const uint32_t m1 = trunc_hi(r1);
            const uint32_t l1 = __builtin_bit_cast(uint32_t, r1 - __builtin_bit_cast(float, m1));
            const bool pl = u < 96;
            lds_char* dp = pl ? hnext + (row * FS_HR + u) * 2 : trashc;
            *reinterpret_cast<__attribute__((address_space(3))) uint16_t*>(dp) = (uint16_t)(h1 >> 16);
            *reinterpret_cast<__attribute__((address_space(3))) uint16_t*>(dp + (pl ? FS_HPL : 0)) = (uint16_t)(m1 >> 16);
            *reinterpret_cast<__attribute__((address_space(3))) uint16_t*>(dp + (pl ? 2 * FS_HPL : 0)) = (uint16_t)(l1 >> 16);
            const bool tl4 = u >= 96 && u < FH;
            lds_char* tp = tl4 ? hnext + 3 * FS_HPL + (row * 4 + (u - 96)) * 4 : trashc;
            *reinterpret_cast<__attribute__((address_space(3))) float*>(tp) = hv;
          }
          st1(hv, rh, v1, 0);
        }
      }
      xp.to_lds(xb + ((t + 1) & 1) * 32 * GX::LR, trash);
      lds_barrier();
    }
  }
}

// ------------------------------------------------------------------------------------------
// The split forward on 8 waves, two per SIMD: lstmf_fwds2_kernel
// ------------------------------------------------------------------------------------------
// lstmf_fwds_kernel runs one wave per SIMD, and each wave alternates an MFMA chain (one row half of its 7
// tiles) with that half's gate math: the matrix pipe idles during the gate math and the VALU during the
// chain.  Here the 25 real gate-interleaved tiles (units 4 gt .. 4 gt + 3 for tile gt; the 3 padding tiles
// of the 4-wave layout are gone) go to 8 waves by columns, wave 0 tiles 0..3 and wave v > 0 tiles 3 v + 1 ..
// 3 v + 3, so the two waves v, v + 4 of a SIMD carry 7 / 6 / 6 / 6 tiles and the hardware interleaves one
// wave's gate math with the other's MFMAs.  256 registers per wave: U's planes stay pinned (36 per tile),
// W^T moves to LDS (25 tiles x 2 x 1 KiB, one ds_read_b128 per tile and four k-steps, read per row half
// like lstmf_fwd_kernel's wl).  The per-tile arithmetic, its order and the addresses are lstmf_fwds_kernel's
// -- tile gt is tile gt % 7 of wave gt / 7 there -- so hs, both tapes and hds are bitwise that kernel's.
// Each tile count is its own straight-line instantiation behind one branch on the wave index at kernel
// entry (no wave-uniform tile guard between an MFMA and the read of its result).
// SKEW, how the two waves of a SIMD get out of phase after the step barrier (bit 0: waves 4..7 run their
// MFMA chains at s_setprio 1; bit 1: waves 4..7 take the row halves in the opposite order).  Both measured
// neutral or slower than plain age arbitration (profiles/fwd_two_wave/README.md), so the knob is off.
#ifndef HFREP_FWDS2_SKEW
#define HFREP_FWDS2_SKEW 0
#endif
constexpr int F2_TILES = 25;
// a product rounded to fp32 on its own: opaque to the compiler, so -ffp-contract=fast cannot fuse it into a
// neighbouring add (explicit fmaf calls are the only fused operations of the cell math below)
__device__ __forceinline__ float f2_rnd(float v) {
  asm("" : "+v"(v));
  return v;
}
template <int KX>
constexpr size_t fwds2_smem() {
  return (size_t)(2 * 32 * FGeo<KX>::LR + 4) * 4 + 2 * FS_HB + (size_t)F2_TILES * FGeo<KX>::NJ * 64 * 16;
}

template <int ACT, int KX, bool TAPE, bool TAN, int NT, bool HI, bool FLIP>
__device__ __forceinline__ void fwds2_run(const float* __restrict__ x, const float* __restrict__ W,
                                          const float* __restrict__ bias, const float* __restrict__ U,
                                          const float* __restrict__ ptape, float* __restrict__ hs,
                                          float* __restrict__ tape, int B, int Tn, float* fsm, int v) {
  using GX = FGeo<KX>;
  float* xb = fsm;                                                 // [2][32 * LRX] fp32, K-permuted
  float* trash = xb + 2 * 32 * GX::LR;                              // [4] out-of-range writes
  lds_char* hb = (lds_char*)(trash + 4);                            // [2][FS_HB] h planes + tail
  f32x4* wl = (f32x4*)(hb + 2 * FS_HB);                             // [25 tiles][NJ][64 lanes] W^T k-steps 4 j .. 4 j + 3
  const int tid = threadIdx.x, lane = tid & 63;
  const int q = lane & 3, g = lane >> 4, j4 = (lane & 15) >> 2;
  const int t0 = v ? 3 * v + 1 : 0;  // first tile of this wave (uniform)
  const int ub = 4 * t0 + j4;        // unit of tile 0 in this lane's MFMA column; tile n adds 4 n
  const int nrb = (B + 31) / 32;
  const int flip = (FLIP && v >= 4) ? 1 : 0;

  for (int i = tid; i < 2 * 32 * GX::LR; i += 512) xb[i] = 0.f;

  constexpr float GSC = ACT == ACT_TANH ? -2.f * kLog2e : ACT == ACT_SIGMOID ? -kLog2e : 1.f;
  const float sc = TAN ? 1.f : (q == 2 ? GSC : -kLog2e);
  bf16x8 up[3][NT][3];
  float ut[NT], bq[NT];
  int tsl[NT];  // tape slot of tile n, row half 0: the 4-wave kernel's (w, n) = (gt / 7, gt % 7) (bytes, uniform)
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int cl = q * FH + ub + 4 * n;  // < 400: every tile is real
    tsl[n] = ftape_lane((t0 + n) / FNT, 0) + (((t0 + n) % FNT) * FT_SLOT) * 4;
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) {
      uint32_t hh[8], mm[8], ll[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 32 * ks + 8 * g + j;  // < 96
        const float u_ = f2_rnd(U[k * FG + cl] * sc);  // (rounded before the split, as there)
        const uint32_t h = trunc_hi(u_);
        const float r1 = u_ - __builtin_bit_cast(float, h);
        const uint32_t m = trunc_hi(r1);
        const float r2 = r1 - __builtin_bit_cast(float, m);
        hh[j] = h; mm[j] = m; ll[j] = __builtin_bit_cast(uint32_t, r2);
      }
      uint4 ph, pm, pl;
      ph.x = __builtin_amdgcn_perm(hh[1], hh[0], 0x07060302u); ph.y = __builtin_amdgcn_perm(hh[3], hh[2], 0x07060302u);
      ph.z = __builtin_amdgcn_perm(hh[5], hh[4], 0x07060302u); ph.w = __builtin_amdgcn_perm(hh[7], hh[6], 0x07060302u);
      pm.x = __builtin_amdgcn_perm(mm[1], mm[0], 0x07060302u); pm.y = __builtin_amdgcn_perm(mm[3], mm[2], 0x07060302u);
      pm.z = __builtin_amdgcn_perm(mm[5], mm[4], 0x07060302u); pm.w = __builtin_amdgcn_perm(mm[7], mm[6], 0x07060302u);
      pl.x = __builtin_amdgcn_perm(ll[1], ll[0], 0x07060302u); pl.y = __builtin_amdgcn_perm(ll[3], ll[2], 0x07060302u);
      pl.z = __builtin_amdgcn_perm(ll[5], ll[4], 0x07060302u); pl.w = __builtin_amdgcn_perm(ll[7], ll[6], 0x07060302u);
      up[ks][n][0] = __builtin_bit_cast(bf16x8, ph);
      up[ks][n][1] = __builtin_bit_cast(bf16x8, pm);
      up[ks][n][2] = __builtin_bit_cast(bf16x8, pl);
      // (no AGPR pin: a kernel that names AGPRs gets its 256 registers as 128 V + 128 A and spills)
#pragma unroll
      for (int p = 0; p < 3; ++p) asm volatile("" : "+v"(up[ks][n][p]));
    }
    ut[n] = U[(96 + g) * FG + cl] * sc;
#pragma unroll
    for (int j = 0; j < GX::NJ; ++j) {
      f32x4 wv;
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        const int k = 4 * (4 * j + s4) + g;
        const float w_ = W[min(k, KX - 1) * FG + cl];
        wv[s4] = k < KX ? w_ * sc : 0.f;
      }
      wl[((t0 + n) * GX::NJ + j) * 64 + lane] = wv;
    }
    const float bv = bias ? bias[cl] : 0.f;
    bq[n] = !TAN ? f2_rnd(bv * sc) : 0.f;
  }
  const bool glin = !TAN && ACT == ACT_LINEAR && q == 2;
  const float am = (ACT == ACT_TANH && q == 2) ? 2.f : 1.f, bm = (ACT == ACT_TANH && q == 2) ? -1.f : 0.f;
  const int ax = (lane & 15) * GX::LR + g * GX::KQ;
  const int ahp = ((lane & 15) * FS_HR + 8 * g) * 2, aht = 3 * FS_HPL + ((lane & 15) * 4 + g) * 4;
  const f32x4* wlw = wl + t0 * GX::NJ * 64 + lane;
  // x_t: the 256 threads of waves 4..7 (the 3-tile waves) load and stage it; the others write the trash word
  FXPart<KX> xp;
  const bool xld = v >= 4;

  for (int rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int row0 = rb * 32;
    const rsrc_t rx = ftile_rsrc(x, row0, B, Tn, KX);
    const rsrc_t rh = ftile_rsrc(hs, row0, B, Tn, FH);
    const rsrc_t rt = ftape_rsrc(TAPE ? tape : nullptr, rb, nrb, Tn);
    const rsrc_t rp = ftape_rsrc(TAN ? ptape : nullptr, rb, nrb, Tn);
    const int vp0 = ((4 * g + q) * Tn * FH + ub) * 4;  // (row 4 g + q, unit ub) in (B,T,H); row half m adds 16 rows
    float cprev[TAN ? 2 : 1][NT];
    if constexpr (TAN) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int n = 0; n < NT; ++n) cprev[i][n] = 0.f;
    }
    float cst[2][NT];  // [i]: the row half this wave takes i-th (half i ^ flip)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int n = 0; n < NT; ++n) cst[i][n] = 0.f;
    xp.set(Tn, tid & 255);
    if (!xld) {
#pragma unroll
      for (int j = 0; j < FXPart<KX>::NJ; ++j) { xp.goff[j] = kOOB; xp.lpos[j] = -1; }
    }
    xp.load(rx, Tn, 0, true);
    for (int i = tid; i < FS_HB / 16; i += 512)
      reinterpret_cast<__attribute__((address_space(3))) u32x4_t*>(hb)[i] = u32x4_t{0, 0, 0, 0};
    xp.to_lds(xb, trash);
    __syncthreads();
    for (int t = 0; t < Tn; ++t) {
      const float* xcur = xb + (t & 1) * 32 * GX::LR;
      const lds_char* hcur = hb + (t & 1) * FS_HB;
      lds_char* hnext = hb + ((t + 1) & 1) * FS_HB;
      xp.load(rx, Tn, t + 1, t + 1 < Tn);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int m = i ^ flip;  // (uniform)
        f32x4 pg[TAN ? NT : 1];
        float pc[TAN ? NT : 1];
        const int p1 = vp0 + (16 * m * Tn + t) * FH * 4;
        const int tb = t * FT_STEP * 4 + m * ftape_slot(1, 0);  // (uniform)
        if constexpr (TAN) {
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            pg[n] = ld4(rp, lane * 16 + (tb + tsl[n]));
            pc[n] = ld1(rp, (256 + lane) * 4 + (tb + tsl[n]), 0);
          }
        }
        f32x4 acc[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (HI) __builtin_amdgcn_s_setprio(1);
        // ---- z = x_t W (exact fp32) ----
#pragma unroll
        for (int j = 0; j < GX::NJ; ++j) {
          const f32x4 a4 = *reinterpret_cast<const f32x4*>(xcur + ax + 16 * m * GX::LR + 4 * j);
          f32x4 w4[NT];
#pragma unroll
          for (int n = 0; n < NT; ++n) w4[n] = wlw[(n * GX::NJ + j) * 64];
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) {
            const int ks = 4 * j + s4;
            if (ks >= GX::KS) break;
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[n] = mma4(a4[s4], w4[n][s4], acc[n]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        // ---- + h_{t-1} U: the split k < 96 and the exact fp32 tail, chained into acc ----
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) {
          const lds_char* ar = hcur + ahp + 16 * m * FS_HR * 2 + 64 * ks;
          const bf16x8 a[3] = {*reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>(ar),
                               *reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>(ar + FS_HPL),
                               *reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>(ar + 2 * FS_HPL)};
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[n] = mma_split6(a, up[ks][n], acc[n]);
          __builtin_amdgcn_sched_barrier(0);
        }
        {
          const float at = *reinterpret_cast<const __attribute__((address_space(3))) float*>(hcur + aht + 16 * m * 16);
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[n] = mma4(at, ut[n], acc[n]);
        }
        if constexpr (HI) __builtin_amdgcn_s_setprio(0);
        // ---- gate math, cell update, stores (row 16 m + 4 g + q, unit ub + 4 n after the transpose) ----
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          // Every product-sum below is written out, fused (fmaf) or rounded (f2_rnd), as the compiler
          // contracted it in lstmf_fwds_kernel.  That differs between that kernel's tiles n < 4 and n >= 4 (the
          // latter sit behind the padded-unit select): fa picks the form of this tile's owner there.
          const int v1 = p1 + 16 * n;
          const int tg = lane * 16 + (tb + tsl[n]), tc = (256 + lane) * 4 + (tb + tsl[n]);
          const bool fa = (t0 + n) % FNT < 4;  // (uniform)
          const f32x4 zs = acc[n];
          float hv, hr;  // h (or hdot) and its residual below the high bf16 plane
          if constexpr (!TAN) {
            float y[4];
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4) {
              const float s_ = zs[e4] + bq[n];
              const float e = __builtin_fmaf(am, __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(s_)), bm);
              y[e4] = glin ? s_ : e;
            }
            quad_transpose(y, q);
            const float cn = __builtin_fmaf(y[1], cst[i][n], y[0] * y[2]);
            float ca;
            if constexpr (ACT == ACT_TANH) ca = __builtin_fmaf(__builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(GSC * cn)), 2.f, -1.f);
            else if constexpr (ACT == ACT_SIGMOID) ca = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(GSC * cn));
            else ca = cn;
            hv = f2_rnd(y[3] * ca);
            const float hh = __builtin_bit_cast(float, trunc_hi(hv));
            hr = fa ? __builtin_fmaf(y[3], ca, -hh) : hv - hh;
            cst[i][n] = cn;
            if constexpr (TAPE) {
              st4(f32x4{y[0], y[1], y[2], y[3]}, rt, tg);
              st1(cn, rt, tc, 0);
            }
          } else {
            float zd[4] = {zs[0], zs[1], zs[2], zs[3]};
            quad_transpose(zd, q);
            const f32x4 y = pg[n];
            const float idot = y[0] * (1.f - y[0]) * zd[0], fdot = y[1] * (1.f - y[1]) * zd[1];
            const float dg = ACT == ACT_TANH ? __builtin_fmaf(-y[2], y[2], 1.f) : ACT == ACT_SIGMOID ? y[2] * (1.f - y[2]) : 1.f;
            const float gdot = dg * zd[2], odot = y[3] * (1.f - y[3]) * zd[3];
            const float c = pc[n];
            const float ca = act_f(ACT, c);
            const float dc = ACT == ACT_TANH ? __builtin_fmaf(-ca, ca, 1.f) : ACT == ACT_SIGMOID ? ca * (1.f - ca) : 1.f;
            const float yd = y[3] * dc;
            float cdn, hd;
            if (fa) {
              if constexpr (ACT == ACT_LINEAR) {
                cdn = f2_rnd(y[0] * gdot) + __builtin_fmaf(idot, y[2], __builtin_fmaf(fdot, cprev[i][n], y[1] * cst[i][n]));
              } else {
                cdn = __builtin_fmaf(y[0], gdot, f2_rnd(idot * y[2]) + (f2_rnd(y[1] * cst[i][n]) + f2_rnd(fdot * cprev[i][n])));
              }
              hd = f2_rnd(odot * ca) + f2_rnd(yd * cdn);
            } else {
              cdn = __builtin_fmaf(y[0], gdot, __builtin_fmaf(idot, y[2], __builtin_fmaf(y[1], cst[i][n], fdot * cprev[i][n])));
              hd = __builtin_fmaf(odot, ca, yd * cdn);
            }
            cst[i][n] = cdn;
            cprev[i][n] = c;
            hv = hd;
            hr = hv - __builtin_bit_cast(float, trunc_hi(hv));
            st4(f32x4{zd[0], zd[1], zd[2], zd[3]}, rt, tg);
            st1(cdn, rt, tc, 0);
          }
          // h (or hdot) of (row 16 m + 4 g + q, unit u) into the next step's planes (u < 96: tiles < 24) or
          // the fp32 tail (tile 24, the last one of wave 7); the tile index is uniform
          {
            const int row = 16 * m + 4 * g + q;
            if (t0 + n < 24) {
              const uint32_t h1 = trunc_hi(hv);
              const uint32_t m1 = trunc_hi(hr);
              const uint32_t l1 = __builtin_bit_cast(uint32_t, hr - __builtin_bit_cast(float, m1));
              lds_char* dp = hnext + (row * FS_HR + ub + 4 * n) * 2;
              *reinterpret_cast<__attribute__((address_space(3))) uint16_t*>(dp) = (uint16_t)(h1 >> 16);
              *reinterpret_cast<__attribute__((address_space(3))) uint16_t*>(dp + FS_HPL) = (uint16_t)(m1 >> 16);
              *reinterpret_cast<__attribute__((address_space(3))) uint16_t*>(dp + 2 * FS_HPL) = (uint16_t)(l1 >> 16);
            } else {
              *reinterpret_cast<__attribute__((address_space(3))) float*>(hnext + 3 * FS_HPL + (row * 4 + j4) * 4) = hv;
            }
          }
          st1(hv, rh, v1, 0);
        }
      }
      xp.to_lds(xb + ((t + 1) & 1) * 32 * GX::LR, trash);
      lds_barrier();
    }
  }
}

template <int ACT, int KX, bool TAPE, bool TAN, int SKEW>
__global__ void __launch_bounds__(512, 1)
lstmf_fwds2_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                   const float* __restrict__ U, const float* __restrict__ ptape, float* __restrict__ hs,
                   float* __restrict__ tape, int B, int Tn) {
  static_assert(FGeo<KX>::KS <= 12, "split forward: K <= 48");
  extern __shared__ __attribute__((aligned(16))) float fsm[];
  constexpr bool PRIO = SKEW & 1, FLIP = SKEW & 2;
  const int v = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (v == 0) fwds2_run<ACT, KX, TAPE, TAN, 4, false, FLIP>(x, W, bias, U, ptape, hs, tape, B, Tn, fsm, v);
  else if (!PRIO || v < 4) fwds2_run<ACT, KX, TAPE, TAN, 3, false, FLIP>(x, W, bias, U, ptape, hs, tape, B, Tn, fsm, v);
  else fwds2_run<ACT, KX, TAPE, TAN, 3, true, FLIP>(x, W, bias, U, ptape, hs, tape, B, Tn, fsm, v);
}

// ------------------------------------------------------------------------------------------
// The exact K = 100 forward on 8 waves, two per SIMD: lstmf_fwd2_kernel
// ------------------------------------------------------------------------------------------
// lstmf_fwd_kernel at K = 100 runs one wave per SIMD: per step and row half a chain of 350 exact MFMAs (7
// tiles x 50 k-steps), then the gate math of the 7 tiles, so the matrix pipe idles through every gate phase,
// and every SIMD pays for 7 tiles although only 25 of the 28 are real.  Here the 25 real tiles (tile gt =
// units 4 gt .. 4 gt + 3 = tile gt % 7 of wave gt / 7 there) go to 8 waves, waves v and v + 4 sharing a SIMD,
// so one wave's gate math issues under its partner's MFMA chain.  Ownership is balanced across the SIMDs by row
// half: wave v owns tiles 3 v .. 3 v + 2 for both row halves, and tile 24 is held by waves 0 and 1, wave 0
// running it for row half 0 and wave 1 for row half 1: 7 / 7 / 6 x 6 tile-halves per wave, 13 / 13 / 12 / 12 per
// SIMD (lstmf_fwds2_kernel's ownership by whole columns, 14 / 12 / 12 / 12, was 5-7 % slower per call here; at
// K = 32 it stays, profiles/fwd_balanced/README.md).  Each of the three roles (3 tiles; 3 + tile 24 in half 0;
// 3 + tile 24 in half 1) is its own straight-line instantiation behind one branch on the wave index at kernel
// entry, the tile count of a row half a compile-time function of the role.  256 registers per wave: U^T stays
// in registers (25 per tile); of W^T's 25 k-steps a 3-tile wave keeps the first 13 and waves 0 and 1 the first 5
// (of all four tiles), the rest sit in LDS as one ds_read_b128 per tile and four k-steps.  x_t is staged by
// waves 2, 3, 6, 7 (the SIMDs with 12 tile-halves).  The per-tile arithmetic is lstmf_fwd_kernel's: zero
// accumulator, the 25 x W k-steps, the 25 h U k-steps, then the bias; the cell math is written out with fmaf /
// f2_rnd in the forms the compiler gave that kernel (scripts/isa_fp_forms.py), so hs, hds and both tapes are
// bitwise its outputs; the tape slots are its slots, those of its three padding tiles stay untouched.
constexpr int F2_NWR3 = 13, F2_NWR4 = 5;  // W^T k-steps in registers: waves 2..7 / waves 0 and 1
constexpr int F2_G3 = (25 - F2_NWR3) / 4, F2_G4 = (25 - F2_NWR4) / 4;  // 1 KiB groups of 4 k-steps in LDS per tile
static_assert(F2_NWR3 + 4 * F2_G3 == 25 && F2_NWR4 + 4 * F2_G4 == 25, "W^T k-steps in LDS come in fours");
// tile n of a wave relative to its first tile t0: its own three, then tile 24 (roles 1 and 2: waves 0 and 1,
// t0 = 0 and 3)
template <int ROLE>
__device__ __forceinline__ constexpr int f2_rel(int n) { return n < 3 ? n : 24 - 3 * (ROLE - 1); }
// first LDS group of tile gt: tiles 0..5 and 24 (waves 0 and 1) take F2_G4 groups each and come first, tile 24
// (one copy, read by both waves) behind tile 5; the others take F2_G3
__device__ __forceinline__ constexpr int f2_woff(int gt) {
  return gt < 6 ? F2_G4 * gt : gt == 24 ? F2_G4 * 6 : F2_G4 * 7 + F2_G3 * (gt - 6);
}
constexpr size_t fwd2_smem() {
  return (size_t)(2 * 32 * (FGeo<100>::LR + FGeo<FH>::LR) + 4) * 4 + (size_t)(F2_G4 * 7 + F2_G3 * 18) * 1024;
}

// one wave: tiles t0 .. t0 + 2 and, for ROLE 1 / 2, tile 24 in row half ROLE - 1
template <int ACT, bool TAPE, bool TAN, int ROLE>
__device__ __forceinline__ void fwd2_run(const float* __restrict__ x, const float* __restrict__ W,
                                         const float* __restrict__ bias, const float* __restrict__ U,
                                         const float* __restrict__ ptape, float* __restrict__ hs,
                                         float* __restrict__ tape, int B, int Tn, float* fsm, int v) {
  constexpr int KX = 100;
  using GX = FGeo<KX>;
  using GH = FGeo<FH>;
  constexpr bool BIG = ROLE != 0;
  constexpr int NT = BIG ? 4 : 3;  // tiles held
  constexpr int NWR = BIG ? F2_NWR4 : F2_NWR3, NG = BIG ? F2_G4 : F2_G3;
  static_assert(GX::KS == 25 && GH::KS == 25 && ROLE >= 0 && ROLE <= 2, "tile plan of the K = 100 layer");
  float* xb = fsm;                         // [2][32 * LRX]
  float* hb = xb + 2 * 32 * GX::LR;        // [2][32 * LRH]
  float* trash = hb + 2 * 32 * GH::LR;     // [4] out-of-range x writes
  f32x4* wl = (f32x4*)(trash + 4);         // [f2_woff(tile) + group][64 lanes]: W^T k-steps NWR + 4 group ..
  const int tid = threadIdx.x, lane = tid & 63;
  const int q = lane & 3, g = lane >> 4, j4 = (lane & 15) >> 2;
  const int t0 = BIG ? 3 * (ROLE - 1) : 3 * v;  // first tile of this wave (uniform; a constant for waves 0 and 1)
  const int nrb = (B + 31) / 32;

  for (int i = tid; i < 2 * 32 * (GX::LR + GH::LR); i += 512) fsm[i] = 0.f;

  constexpr float GSC = ACT == ACT_TANH ? -2.f * kLog2e : ACT == ACT_SIGMOID ? -kLog2e : 1.f;
  const float sc = TAN ? 1.f : (q == 2 ? GSC : -kLog2e);
  float uf[GH::KS][NT], wf[NWR][NT], bq[NT];
  int tsl[NT];  // tape slot of tile n, row half 0: the 4-wave kernel's (w, n) = (gt / 7, gt % 7) (bytes, uniform)
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int gt = t0 + f2_rel<ROLE>(n);
    const int cl = q * FH + 4 * gt + j4;  // < 400: every tile is real
    tsl[n] = ftape_lane(gt / FNT, 0) + ((gt % FNT) * FT_SLOT) * 4;
#pragma unroll
    for (int ks = 0; ks < GH::KS; ++ks) {
      uf[ks][n] = U[(4 * ks + g) * FG + cl] * sc;
      // (no AGPR pin: a kernel that names AGPRs gets its 256 registers as 128 V + 128 A and spills)
      asm volatile("" : "+v"(uf[ks][n]));
    }
#pragma unroll
    for (int ks = 0; ks < NWR; ++ks) {
      wf[ks][n] = W[(4 * ks + g) * FG + cl] * sc;
      asm volatile("" : "+v"(wf[ks][n]));
    }
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) {
      f32x4 wv;
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) wv[s4] = W[(4 * (NWR + 4 * gi + s4) + g) * FG + cl] * sc;
      if (n < 3 || ROLE == 1) wl[(f2_woff(gt) + gi) * 64 + lane] = wv;  // (tile 24's one copy: wave 0 writes it)
    }
    const float bv = bias ? bias[cl] : 0.f;
    bq[n] = !TAN ? f2_rnd(bv * sc) : 0.f;
  }
  const bool glin = !TAN && ACT == ACT_LINEAR && q == 2;
  const float am = q == 2 ? 2.f : 1.f, bm = q == 2 ? -1.f : 0.f;  // (tanh)
  // LDS element offsets: A-fragment reads (row l & 15, k-group g) and the h write of (row 4 g + q, unit 4 gt + j4)
  const int ax = (lane & 15) * GX::LR + g * GX::KQ, ah = (lane & 15) * GH::LR + g * GH::KQ;
  const int hw = (4 * g + q) * GH::LR + j4 * GH::KQ + t0;
  const f32x4* wlw = wl + f2_woff(t0) * 64 + lane;  // tile n: + wrel(n) * 64
  constexpr int WR24 = BIG ? f2_woff(24) - f2_woff(3 * (ROLE - 1)) : 0;  // tile 24 from t0 (waves 0 and 1 only)
  auto wrel = [](int n) constexpr { return n < 3 ? n * NG : WR24; };  // (n = 3 occurs in those two roles only)
  // x_t: the 256 threads of waves 2, 3, 6, 7 load and stage it; waves 4 and 5 write the trash word, waves 0 and 1
  // have no loader
  FXPart<KX> xp;
  const bool xld = (v & 2) != 0;
  const int xtid = (((v >> 2) << 1) | (v & 1)) * 64 + lane;  // loaders: 0..255
  __syncthreads();  // (the zero fill above, before any wave stages x_0)

  for (int rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int row0 = rb * 32;
    const rsrc_t rx = ftile_rsrc(x, row0, B, Tn, KX);
    const rsrc_t rh = ftile_rsrc(hs, row0, B, Tn, FH);
    const rsrc_t rt = ftape_rsrc(TAPE ? tape : nullptr, rb, nrb, Tn);
    const rsrc_t rp = ftape_rsrc(TAN ? ptape : nullptr, rb, nrb, Tn);
    const int vp0 = ((4 * g + q) * Tn * FH + 4 * t0 + j4) * 4;  // (row 4 g + q, unit of tile 0) in (B,T,H); half m adds 16 rows
    float cprev[TAN ? 2 : 1][NT];
    if constexpr (TAN) {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) cprev[m][n] = 0.f;
    }
    float cst[2][NT];  // (tile 24, n = 3: only the entries of row half ROLE - 1 are live)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n) cst[m][n] = 0.f;
    if constexpr (!BIG) {
      xp.set(Tn, xtid);
      if (!xld) {
#pragma unroll
        for (int j = 0; j < FXPart<KX>::NJ; ++j) { xp.goff[j] = kOOB; xp.lpos[j] = -1; }
      }
      xp.load(rx, Tn, 0, true);
    }
    for (int i = tid; i < 32 * GH::LR; i += 512) hb[i] = 0.f;  // h_{-1} = 0
    if constexpr (!BIG) xp.to_lds(xb, trash);
    __syncthreads();
    for (int t = 0; t < Tn; ++t) {
      const float* xcur = xb + (t & 1) * 32 * GX::LR;
      const float* hcur = hb + (t & 1) * 32 * GH::LR;
      float* hnext = hb + ((t + 1) & 1) * 32 * GH::LR;
      if constexpr (!BIG) xp.load(rx, Tn, t + 1, t + 1 < Tn);  // x_{t+1}: lands during this step's MFMAs
      // one row half: NH tiles, a compile-time function of the role (tile 24 in row half ROLE - 1 only)
      auto half = [&](auto M_) {
        constexpr int m = decltype(M_)::value;
        constexpr int NH = (BIG && m == ROLE - 1) ? 4 : 3;
        f32x4 pg[TAN ? NH : 1];
        float pc[TAN ? NH : 1];
        const int p1 = vp0 + (16 * m * Tn + t) * FH * 4;
        const int tb = t * FT_STEP * 4 + ftape_slot(m, 0);  // (uniform)
        if constexpr (TAN) {
          // the primal gates and c_t of this lane's (row, unit): issued before this half's MFMAs
#pragma unroll
          for (int n = 0; n < NH; ++n) {
            pg[n] = ld4(rp, lane * 16 + (tb + tsl[n]));
            pc[n] = ld1(rp, (256 + lane) * 4 + (tb + tsl[n]), 0);
          }
        }
        f32x4 acc[NH];
#pragma unroll
        for (int n = 0; n < NH; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
        // ---- z = x_t W: k-steps < NWR from registers, then one b128 group per tile and four k-steps ----
        f32x4 w4[NH];
#pragma unroll
        for (int j = 0; j < GX::NJ; ++j) {
          const f32x4 a4 = *reinterpret_cast<const f32x4*>(xcur + ax + 16 * m * GX::LR + 4 * j);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int ks = 4 * j + s;
            if (ks >= GX::KS) break;
            if (ks >= NWR && (ks - NWR) % 4 == 0) {
#pragma unroll
              for (int n = 0; n < NH; ++n) w4[n] = wlw[(wrel(n) + (ks - NWR) / 4) * 64];
            }
#pragma unroll
            for (int n = 0; n < NH; ++n) {
              const float bw = ks < NWR ? wf[ks < NWR ? ks : 0][n] : w4[n][(ks >= NWR ? ks - NWR : 0) & 3];
              acc[n] = mma4(a4[s], bw, acc[n]);
            }
          }
          __builtin_amdgcn_sched_barrier(0);  // bound the live range of hoisted fragment reads
        }
        // ---- + h_{t-1} U ----
#pragma unroll
        for (int j = 0; j < GH::NJ; ++j) {
          const f32x4 a4 = *reinterpret_cast<const f32x4*>(hcur + ah + 16 * m * GH::LR + 4 * j);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int ks = 4 * j + s;
            if (ks >= GH::KS) break;
#pragma unroll
            for (int n = 0; n < NH; ++n) acc[n] = mma4(a4[s], uf[ks][n], acc[n]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        // ---- gate math, cell update, stores (row 16 m + 4 g + q, unit 4 gt + j4 after the transpose) ----
#pragma unroll
        for (int n = 0; n < NH; ++n) {
          // Every product-sum is written out, fused (fmaf) or rounded (f2_rnd), as the compiler contracted it
          // in lstmf_fwd_kernel<ACT, 100>: one form per value everywhere, except the tangent's cdot in row
          // half 0 of that kernel's tile 4 of every wave (global tiles 4, 11, 18; odd, uniform)
          const int v1 = p1 + 16 * f2_rel<ROLE>(n);
          const int tg = lane * 16 + (tb + tsl[n]), tc = (256 + lane) * 4 + (tb + tsl[n]);
          const f32x4 zs = acc[n];
          float hv;
          if constexpr (!TAN) {
            float y[4];
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4) {
              const float s_ = zs[e4] + bq[n];
              const float r_ = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(s_));
              float e = r_;
              if constexpr (ACT == ACT_TANH) e = __builtin_fmaf(am, r_, bm);
              y[e4] = glin ? s_ : e;
            }
            quad_transpose(y, q);  // y = (i, f, g, o) of (row, unit)
            const float cn = __builtin_fmaf(y[1], cst[m][n], y[0] * y[2]);
            float ca;
            if constexpr (ACT == ACT_TANH) ca = __builtin_fmaf(__builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(GSC * cn)), 2.f, -1.f);
            else if constexpr (ACT == ACT_SIGMOID) ca = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(GSC * cn));
            else ca = cn;
            hv = y[3] * ca;
            cst[m][n] = cn;
            if constexpr (TAPE) {
              st4(f32x4{y[0], y[1], y[2], y[3]}, rt, tg);
              st1(cn, rt, tc, 0);
            }
          } else {
            float zd[4] = {zs[0], zs[1], zs[2], zs[3]};
            quad_transpose(zd, q);  // zdot of (row, unit) for all four gates
            const f32x4 y = pg[n];
            const float idot = y[0] * (1.f - y[0]) * zd[0], fdot = y[1] * (1.f - y[1]) * zd[1];
            const float dg = ACT == ACT_TANH ? __builtin_fmaf(-y[2], y[2], 1.f) : ACT == ACT_SIGMOID ? y[2] * (1.f - y[2]) : 1.f;
            const float gdot = dg * zd[2], odot = y[3] * (1.f - y[3]) * zd[3];
            const float c = pc[n];
            const float ca = act_f(ACT, c);
            const float dc = ACT == ACT_TANH ? __builtin_fmaf(-ca, ca, 1.f) : ACT == ACT_SIGMOID ? ca * (1.f - ca) : 1.f;
            const float yd = y[3] * dc;
            const float fc = __builtin_fmaf(fdot, cprev[m][n], y[1] * cst[m][n]);
            float cdn = __builtin_fmaf(y[0], gdot, __builtin_fmaf(idot, y[2], fc));
            if (m == 0 && (t0 + f2_rel<ROLE>(n)) % FNT == 4) {  // (uniform)
              if constexpr (ACT == ACT_LINEAR) cdn = f2_rnd(y[0] * gdot) + (f2_rnd(idot * y[2]) + (f2_rnd(fdot * cprev[m][n]) + f2_rnd(y[1] * cst[m][n])));
              else cdn = __builtin_fmaf(y[0], gdot, f2_rnd(idot * y[2]) + fc);
            }
            hv = __builtin_fmaf(odot, ca, yd * cdn);
            cst[m][n] = cdn;
            cprev[m][n] = c;
            st4(f32x4{zd[0], zd[1], zd[2], zd[3]}, rt, tg);
            st1(cdn, rt, tc, 0);
          }
          hnext[hw + 16 * m * GH::LR + f2_rel<ROLE>(n)] = hv;  // K-permuted: unit u at (u & 3) * KQ + (u >> 2)
          st1(hv, rh, v1, 0);
        }
      };
      half(I0{});
      half(I1{});
      if constexpr (!BIG) xp.to_lds(xb + ((t + 1) & 1) * 32 * GX::LR, trash);
      lds_barrier();
    }
  }
}

template <int ACT, int KX, bool TAPE, bool TAN>
__global__ void __launch_bounds__(512, 1)
lstmf_fwd2_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                  const float* __restrict__ U, const float* __restrict__ ptape, float* __restrict__ hs,
                  float* __restrict__ tape, int B, int Tn) {
  static_assert(KX == 100, "the eight-wave exact forward is the K = 100 layer's");
  extern __shared__ __attribute__((aligned(16))) float fsm[];
  const int v = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (v == 0) fwd2_run<ACT, TAPE, TAN, 1>(x, W, bias, U, ptape, hs, tape, B, Tn, fsm, v);
  else if (v == 1) fwd2_run<ACT, TAPE, TAN, 2>(x, W, bias, U, ptape, hs, tape, B, Tn, fsm, v);
  else fwd2_run<ACT, TAPE, TAN, 0>(x, W, bias, U, ptape, hs, tape, B, Tn, fsm, v);
}

// ------------------------------------------------------------------------------------------
// BPTT with the recurrent product on the bf16 matrix pipe: lstmf_bwds_kernel
// ------------------------------------------------------------------------------------------
// lstmf_bwdp_kernel's step is bound by dh_rec = dz_{t+1} U^T on the exact fp32 MFMA (400 16x16x4
// MFMAs per MFMA-role wave and step).  Here the product is the exact three-term bf16 split (dz and U^T
// each h + m + l; six products lh hl mm mh hm hh, the dropped terms <= 2^-24 of each product) on
// v_mfma_f32_16x16x32_bf16: 13 k-steps x 2 tiles x 6 = 156 MFMAs per half tile and wave, ~1/2.5 of the
// fp32 pipe time.  The matrix work and the cell math are then of the same size, so the roles merge:
// 4 waves (one per SIMD, 512 registers), wave w does the MFMAs of output tiles 2 w, 2 w + 1 AND the
// cells of units 28 w .. 28 w + 27, one cell after each of the first 7 k-steps, so the VALU issues the
// cell math of one row half while the matrix pipe runs the other half's product.  The row-half pipeline
// is lstmf_bwdp_kernel's:
//   P1(t): B(0, t) + A(1, t)      P2(t): B(1, t) + A(0, t - 1)
// The dz tile has two images: the fp32 rows (dZ's coalesced HBM stores, as before) and three bf16
// planes in the gate-interleaved column order k = 4 u + q (a cell writes its four gates as one 8-byte
// word per plane), row stride 424 (conflict-free ds_read_b128).  B[k][j] = U[j][(k & 3) H + (k >> 2)],
// k >= 400 zero: 312 registers per wave, 252 of them pinned in AGPRs.  One tape register set: a cell's
// loads for the other half's next use are issued as soon as it has consumed the set.
// AHD: the total adjoint of every h_t (dht = dH_t + dz_{t+1} U^T) also leaves as a row-major (B, T, H)
// tensor aH: the single-stream tangent reverse (lstmf_tbwd1_kernel) reads it as its tangent-stream
// adjoint.  One dword store per cell behind the cell's next tape loads, addressed like the cell's dH load
// (lane row in voffset, step and unit tile in soffset); dZ is bitwise the AHD = false kernel's.
constexpr int BS_LZ = 432;             // dz plane row stride (bf16 elements): 216 dwords
constexpr int BS_PL = 32 * BS_LZ * 2;  // bytes per dz plane (32 rows)

template <int ACT, bool HEAD = false, bool AHD = false>
__global__ void __launch_bounds__(256, 1)
lstmf_bwds_kernel(const float* __restrict__ dH, const float* __restrict__ tape, const float* __restrict__ U,
                  float* __restrict__ dZ, int B, int Tn, const float* __restrict__ hd, const float* __restrict__ hw,
                  float* __restrict__ aH) {
  extern __shared__ __attribute__((aligned(16))) float fsm[];
  float* zt = fsm;                                     // fp32 dz tile [32][BZ_LR]: [q][u'] per row
  float* ht = zt + 32 * BZ_LR;                         // dh_rec tile [32][BH_LR]
  float* trash = ht + 32 * BH_LR;                      // [4 * BZ_KQ + 4] padding words, never read
  lds_char* trashp = (lds_char*)(trash + 4 * BZ_KQ);
  lds_char* zp = (lds_char*)(trash + 4 * BZ_KQ + 4);   // dz planes [3][32][BS_LZ] bf16
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = lane & 3, g = lane >> 4, j4 = (lane & 15) >> 2, c16 = lane & 15;
  const int nrb = (B + 31) / 32;
  // U^T planes: B[k = 32 ks + 8 g + j][col 16 (2 w + e) + c16] = U[col][(k & 3) H + (k >> 2)]
  bf16x8 up[2][DS_KS][3];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int col = 16 * (2 * w + e) + c16;
    const bool ok = col < FH;
#pragma unroll
    for (int ks = 0; ks < DS_KS; ++ks) {
      f32x4 v[2];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = min(32 * ks + 8 * g + j, FG - 1);
        const float x = U[(ok ? col : 0) * FG + (k & 3) * FH + (k >> 2)];
        v[j >> 2][j & 3] = (ok && 32 * ks + 8 * g + j < FG) ? x : 0.f;
      }
      uint32_t p0[3][2], p1[3][2];
      split3(v[0], p0);
      split3(v[1], p1);
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        up[e][ks][p] = __builtin_bit_cast(bf16x8, make_uint4(p0[p][0], p0[p][1], p1[p][0], p1[p][1]));
        if (e == 1 || ks < 8) asm volatile("" : "+a"(up[e][ks][p]));
      }
    }
  }
  const int ub = FUW * w + j4;
  const int hr = (4 * g + q) * BH_LR + ub, zw = (4 * g + q) * BZ_LR + ub;  // (+16 m rows, + 4 n units)
  const int zpw = ((4 * g + q) * BS_LZ + 4 * ub) * 2;                    // plane word (+ 32 n bytes)
  const int ao = (c16 * BS_LZ + 8 * g) * 2;  // A fragment: row c16 (+ 16 M), k = 32 ks + 8 g .. + 7
  const RevStore st(tid, Tn);
  const int tl = ftape_lane(w, lane), tcl = ftape_cell(w, lane);
  for (int rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int row0 = rb * 32;
    const rsrc_t rdh = ftile_rsrc(dH, row0, B, Tn, FH), rt = ftape_rsrc(tape, rb, nrb, Tn);
    const rsrc_t rz = ftile_rsrc(dZ, row0, B, Tn, FG);
    const rsrc_t rah = ftile_rsrc(AHD ? aH : nullptr, row0, B, Tn, FH);
    const int nr = min(32, B - row0);
    int vp1[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) vp1[m] = ((16 * m + 4 * g + q) * Tn * FH + ub) * 4;
    // HEAD: the lane rows' head adjoint factors d[row] (0 past B) and the head weight's descriptor
    float hdv[2];
    head_rows<HEAD>(hdv, hd, true, row0, B, g, q);  // (the launcher selects HEAD by hd)
    const rsrc_t rhw = head_rsrc<HEAD>(hw, Tn);
    const int hvo = ub * 4;
    float dc[2][FNT], tc[2][FNT];
    f32x4 tg[FNT];
    float tcp[FNT], tdh[FNT];
    const int T1 = Tn - 1;
#pragma unroll
    for (int n = 0; n < FNT; ++n) {
      const bool tok = unit_ok(w, n);
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        dc[m][n] = 0.f;
        tc[m][n] = ld1(rt, tok ? tcl + T1 * FT_STEP * 4 + ftape_slot(m, n) : kOOB, 0);  // c_{T-1}
      }
      bwdf_tape_load_u<HEAD>(tg[n], tcp[n], tdh[n], rt, rdh, tl, tcl, vp1[0], T1 * FT_STEP * 4 + ftape_slot(0, n),
                             max(T1 - 1, 0) * FT_STEP * 4 + ftape_slot(0, n), T1 * FH * 4 + 16 * n, tok, T1 > 0, hdv[0],
                             rhw, hvo);
    }
    // dz_T = 0 (planes, pad columns k >= 400 included), dh_rec(T - 1) = 0
    for (int i = tid; i < 3 * BS_PL / 16; i += 256)
      reinterpret_cast<__attribute__((address_space(3))) u32x4_t*>(zp)[i] = u32x4_t{0, 0, 0, 0};
    for (int i = tid; i < 32 * BH_LR; i += 256) ht[i] = 0.f;
    __syncthreads();
    // cell adjoint of (row half M, unit tile n) at step t, then the loads for the set's next use
    auto cell = [&](auto M_, int n, float hrec, int t) {
      constexpr int m = decltype(M_)::value;
      const bool tok = unit_ok(w, n);
      f32x4 z4;
      const float dht = bptt_cell<ACT>(z4, dc[m][n], tg[n], tc[m][n], tcp[n], tdh[n], hrec, tok,
                                       zt + zw + 16 * m * BZ_LR + 4 * n, trash);
      // (the plane split and store after the fp32 words, the AHD store last: this statement order keeps the
      // twelve kernels' instruction streams, profiles/lstmf_grad_split/README.md)
      uint32_t p[3][2];
      split3(z4, p);
      planes_store(p, tok ? zp + zpw + 16 * m * BS_LZ * 2 + 32 * n : trashp, tok ? BS_PL : 0);
      tc[m][n] = tcp[n];  // c_{t-1} is the next step's c
      if constexpr (m == 0) {  // next use: B(1, t)
        bwdf_tape_load_u<HEAD>(tg[n], tcp[n], tdh[n], rt, rdh, tl, tcl, vp1[1], t * FT_STEP * 4 + ftape_slot(1, n),
                               max(t - 1, 0) * FT_STEP * 4 + ftape_slot(1, n), t * FH * 4 + 16 * n, tok, t > 0, hdv[1],
                               rhw, hvo);
      } else {  // next use: B(0, t - 1)
        const int tp = t > 0 ? t - 1 : 0;
        bwdf_tape_load_u<HEAD>(tg[n], tcp[n], tdh[n], rt, rdh, tl, tcl, vp1[0], tp * FT_STEP * 4 + ftape_slot(0, n),
                               max(tp - 1, 0) * FT_STEP * 4 + ftape_slot(0, n), tp * FH * 4 + 16 * n, tok && t > 0,
                               tp > 0, hdv[0], rhw, hvo);
      }
      // (rows past B: voffset past the descriptor; padding cells: kOOB)
      if constexpr (AHD) st1(dht, rah, tok ? vp1[m] : kOOB, t * FH * 4 + 16 * n);
    };
    // one half-phase: dz rows of half MA out to HBM, the cells of half 1 - MA at step t, and rows MA of
    // dh_rec = dz[rows MA] U^T (the planes hold dz_{t + 1} there for MA = 1, dz_t for MA = 0)
    auto phase = [&](auto MA_, int t) {
      constexpr int MA = decltype(MA_)::value;
      // rows of half MA of the fp32 dz tile -> dZ
      if constexpr (MA == 1) {
        if (t < T1) st.half<1, false>(zt, rz, Tn, t + 1, nr);
      } else {
        st.half<0, false>(zt, rz, Tn, t, nr);
      }
      float hv[FNT];  // the cells' dh_rec words (rows of half 1 - MA, completed in the previous phase)
#pragma unroll
      for (int n = 0; n < FNT; ++n) hv[n] = ht[hr + 16 * (1 - MA) * BH_LR + 4 * n];
      __builtin_amdgcn_sched_barrier(0);
      f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      const lds_char* ar = zp + ao + 16 * MA * BS_LZ * 2;
      bf16x8 af[2][3];
#pragma unroll
      for (int p = 0; p < 3; ++p) af[0][p] = *reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>(ar + p * BS_PL);
#pragma unroll
      for (int ks = 0; ks < DS_KS; ++ks) {
        if (ks + 1 < DS_KS) {
#pragma unroll
          for (int p = 0; p < 3; ++p)
            af[(ks + 1) & 1][p] = *reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>(ar + p * BS_PL + 64 * (ks + 1));
        }
        const bf16x8(&a)[3] = af[ks & 1];
#pragma unroll
        for (int e = 0; e < 2; ++e) acc[e] = mma_split6(a, up[e][ks], acc[e]);
        if (ks < FNT) cell(std::integral_constant<int, 1 - MA>{}, ks, hv[ks], t);  // (compile-time)
      }
      // one schedule for the whole phase: per k-step its A fragments, then its 12 MFMAs with 3 VALU
      // slots (the cells' math) after each one; loads and LDS stores of the cells go where they fit
#pragma unroll
      for (int ks = 0; ks < DS_KS; ++ks) {
        __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
#pragma unroll
        for (int i = 0; i < 12; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      // rows 16 MA + 4 g + i, column 16 (2 w + e) + c16 (wave 3's second tile is past the 112 units: trash)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const bool ok = 2 * w + e < 7;
        float* hd = ok ? ht + (16 * MA + 4 * g) * BH_LR + 16 * (2 * w + e) + c16 : trash;
        const int hs = ok ? BH_LR : 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) hd[i * hs] = acc[e][i];
      }
      lds_barrier();
    };
    for (int t = T1; t >= 0; --t) {
      phase(I1{}, t);  // P1(t): B(0, t) + A(1, t)
      phase(I0{}, t);  // P2(t): B(1, t) + A(0, t - 1)
    }
    st.half<1, false>(zt, rz, Tn, 0, nr);
    __syncthreads();  // (the tiles are re-zeroed for the next row block)
  }
}

// ------------------------------------------------------------------------------------------
// The split BPTT on 8 waves, two per SIMD: lstmf_bwds2_kernel
// ------------------------------------------------------------------------------------------
// lstmf_bwds_kernel runs one wave per SIMD, and that wave issues its 156 MFMAs, seven cells' VALU and
// transcendentals, the plane split, the tape loads and the dZ stores in program order: every s_waitcnt, LDS
// latency or barrier wait leaves its SIMD idle, and one of the eight dh_rec tiles is padding (units 112..127).
// Here the work goes to 8 waves, waves v and v + 4 sharing a SIMD:
//   * MFMA tiles: wave v < 7 owns the one real 16-column tile v of dh_rec = dz U^T (columns 16 v .. 16 v + 15;
//     tile e of wave w there is tile 2 w + e here) for all 13 k-steps, its U^T planes in 156 registers, one
//     accumulator chain from zero per half-phase in that kernel's order (mma_split6 over ks = 0..12); wave 7 has
//     no tile and the padding tile is gone;
//   * cells: the 25 real cell groups (4 units x 16 rows; group gt = units 4 gt .. 4 gt + 3 = group gt % 7 of wave
//     gt / 7 there) go by threes, wave v < 7 groups 3 v .. 3 v + 2 and wave 7 groups 21 .. 24: a SIMD carries two
//     tiles and six groups (SIMDs 0..2) or one tile and seven groups (SIMD 3), split 3 + 3 or 3 + 4 over its waves;
//   * dZ stores: all on wave 7, the wave without a tile (lane l: the 16-byte chunks l and, l < 36, l + 64 of every
//     row of the half); on the tile waves the store data and addresses cost the registers that U^T needs
//     (profiles/bwds_two_wave/README.md).
// The tape keeps the four-wave lane-native layout and a group addresses its slots, its dH words, the head
// weight and its dz / plane / ht words through its global index.  There is no AHD form: with the h adjoints kept the
// eight-wave kernel measured no clear gain per call (profiles/bwds_two_wave/README.md), so those launches stay on
// lstmf_bwds_kernel under every value of the switch.  The LDS images, the row-half pipeline
//   P1(t): B(0, t) + A(1, t)      P2(t): B(1, t) + A(0, t - 1)
// and the LDS-only barrier per half-phase are lstmf_bwds_kernel's; a cell reads ht words and writes dz words of
// the row half the MFMAs of the phase do not touch, so any ownership of tiles and groups is race-free between two
// barriers.  Each role (a tile and 3 groups; no tile, 4 groups and the stores) is its own straight-line
// instantiation behind one branch on the wave index at kernel entry.  dZ is bitwise lstmf_bwds_kernel's
// (tests/test_bwds_two_wave_gpu.py).

// the dz tile -> dZ[:, t, :] from ONE wave: lane l owns the 16-byte chunks l and l + 64 (l < 36; the others store
// out of range) of every row, the row in the uniform offset
struct RevStoreW {
  int lo[2], go[2];
  __device__ __forceinline__ RevStoreW(int lane, int Tn) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bool ok = lane + 64 * j < 100;
      const int ch = ok ? lane + 64 * j : lane, qq = ch / 25, c = ch - 25 * qq;
      lo[j] = qq * BZ_KQ + 4 * c;
      go[j] = ok ? (qq * FH + 4 * c) * 4 : kOOB;
    }
  }
  // rows of half M of `tile` (holding dz at step ts) -> dZ[:, ts, :], as RevStore::half
  template <int M>
  __device__ __forceinline__ void half(const float* tile, rsrc_t rz, int Tn, int ts, int nr) const {
#pragma unroll
    for (int r = 16 * M; r < 16 * M + 16; ++r) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(tile + lo[j] + r * BZ_LR);
        st16(v, rz, r < nr, go[j], (r * Tn + ts) * FG * 4);
      }
    }
  }
};

#ifndef HFREP_BWDS2_NAF
// A-fragment register sets of a tile wave: 2 (the next k-step's reads under this one's MFMAs) spills 320-500 B
#define HFREP_BWDS2_NAF 1
#endif
template <int ACT, bool HEAD, int NG, bool TILE, bool ST>
__device__ __forceinline__ void bwds2_run(const float* __restrict__ dH, const float* __restrict__ tape,
                                          const float* __restrict__ U, float* __restrict__ dZ, int B, int Tn,
                                          const float* __restrict__ hd, const float* __restrict__ hw, float* fsm,
                                          int v) {
  float* zt = fsm;                                     // fp32 dz tile [32][BZ_LR]: [q][u'] per row
  float* ht = zt + 32 * BZ_LR;                         // dh_rec tile [32][BH_LR]
  float* trash = ht + 32 * BH_LR;                      // [4 * BZ_KQ + 4] padding words (every group here is real)
  lds_char* zp = (lds_char*)(trash + 4 * BZ_KQ + 4);   // dz planes [3][32][BS_LZ] bf16
  const int tid = threadIdx.x, lane = tid & 63;
  const int q = lane & 3, g = lane >> 4, j4 = (lane & 15) >> 2, c16 = lane & 15;
  const int nrb = (B + 31) / 32;
  const int g0 = 3 * v;  // first cell group of this wave (uniform)
  // U^T planes of tile v: B[k = 32 ks + 8 g + j][col 16 v + c16] = U[col][(k & 3) H + (k >> 2)]
  bf16x8 up[TILE ? DS_KS : 1][3];
  if constexpr (TILE) {
    const int col = 16 * v + c16;
    const bool ok = col < FH;
#pragma unroll
    for (int ks = 0; ks < DS_KS; ++ks) {
      f32x4 uv[2];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = min(32 * ks + 8 * g + j, FG - 1);
        const float x = U[(ok ? col : 0) * FG + (k & 3) * FH + (k >> 2)];
        uv[j >> 2][j & 3] = (ok && 32 * ks + 8 * g + j < FG) ? x : 0.f;
      }
      uint32_t p0[3][2], p1[3][2];
      split3(uv[0], p0);
      split3(uv[1], p1);
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        up[ks][p] = __builtin_bit_cast(bf16x8, make_uint4(p0[p][0], p0[p][1], p1[p][0], p1[p][1]));
        // (no AGPR pin: a kernel that names AGPRs gets its 256 registers as 128 V + 128 A and spills)
        asm volatile("" : "+v"(up[ks][p]));
      }
    }
  }
  const int ub = 4 * g0 + j4;  // unit of group 0 in this lane; group k adds 4 k
  const int hr = (4 * g + q) * BH_LR + ub, zw = (4 * g + q) * BZ_LR + ub;  // (+16 m rows, + 4 k units)
  const int zpw = ((4 * g + q) * BS_LZ + 4 * ub) * 2;                    // plane word (+ 32 k bytes)
  const int ao = (c16 * BS_LZ + 8 * g) * 2;  // A fragment: row c16 (+ 16 M), k = 32 ks + 8 g .. + 7
  const RevStoreW st(lane, Tn);              // (used by the store role alone)
  const int tl = lane * 16, tcl = (256 + lane) * 4;
  int tsl[NG];  // tape slot of group k, row half 0: the four-wave kernel's (w, n) = (gt / 7, gt % 7) (bytes, uniform)
#pragma unroll
  for (int k = 0; k < NG; ++k) tsl[k] = ftape_lane((g0 + k) / FNT, 0) + ftape_slot(0, (g0 + k) % FNT);
  for (int rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int row0 = rb * 32;
    const rsrc_t rdh = ftile_rsrc(dH, row0, B, Tn, FH), rt = ftape_rsrc(tape, rb, nrb, Tn);
    const rsrc_t rz = ftile_rsrc(dZ, row0, B, Tn, FG);
    const int nr = min(32, B - row0);
    int vp1[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) vp1[m] = ((16 * m + 4 * g + q) * Tn * FH + ub) * 4;
    float hdv[2];
    head_rows<HEAD>(hdv, hd, true, row0, B, g, q);  // (the launcher selects HEAD by hd)
    const rsrc_t rhw = head_rsrc<HEAD>(hw, Tn);
    const int hvo = ub * 4;
    float dc[2][NG], tc[2][NG];
    f32x4 tg[NG];
    float tcp[NG], tdh[NG];
    const int T1 = Tn - 1;
#pragma unroll
    for (int k = 0; k < NG; ++k) {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        dc[m][k] = 0.f;
        tc[m][k] = ld1(rt, tcl, T1 * FT_STEP * 4 + m * ftape_slot(1, 0) + tsl[k]);  // c_{T-1}
      }
      bwdf_tape_load_u<HEAD>(tg[k], tcp[k], tdh[k], rt, rdh, tl, tcl, vp1[0], T1 * FT_STEP * 4 + tsl[k],
                             max(T1 - 1, 0) * FT_STEP * 4 + tsl[k], T1 * FH * 4 + 16 * k, true, T1 > 0, hdv[0], rhw, hvo);
    }
    // dz_T = 0 (planes, pad columns k >= 400 included), dh_rec(T - 1) = 0
    for (int i = tid; i < 3 * BS_PL / 16; i += 512)
      reinterpret_cast<__attribute__((address_space(3))) u32x4_t*>(zp)[i] = u32x4_t{0, 0, 0, 0};
    for (int i = tid; i < 32 * BH_LR; i += 512) ht[i] = 0.f;
    __syncthreads();
    // cell adjoint of (row half M, group k) at step t, then the loads for the set's next use
    auto cell = [&](auto M_, int k, float hrec, int t) {
      constexpr int m = decltype(M_)::value;
      f32x4 z4;
      bptt_cell<ACT>(z4, dc[m][k], tg[k], tc[m][k], tcp[k], tdh[k], hrec, true, zt + zw + 16 * m * BZ_LR + 4 * k, trash);
      uint32_t p[3][2];
      split3(z4, p);
      planes_store(p, zp + zpw + 16 * m * BS_LZ * 2 + 32 * k, BS_PL);
      tc[m][k] = tcp[k];  // c_{t-1} is the next step's c
      const int sl = (1 - m) * ftape_slot(1, 0) + tsl[k];  // the set's next use is the other row half
      if constexpr (m == 0) {  // next use: B(1, t)
        bwdf_tape_load_u<HEAD>(tg[k], tcp[k], tdh[k], rt, rdh, tl, tcl, vp1[1], t * FT_STEP * 4 + sl,
                               max(t - 1, 0) * FT_STEP * 4 + sl, t * FH * 4 + 16 * k, true, t > 0, hdv[1], rhw, hvo);
      } else {  // next use: B(0, t - 1)
        const int tp = t > 0 ? t - 1 : 0;
        bwdf_tape_load_u<HEAD>(tg[k], tcp[k], tdh[k], rt, rdh, tl, tcl, vp1[0], tp * FT_STEP * 4 + sl,
                               max(tp - 1, 0) * FT_STEP * 4 + sl, tp * FH * 4 + 16 * k, t > 0, tp > 0, hdv[0], rhw, hvo);
      }
    };
    // one half-phase: dz rows of half MA out to HBM (store role), the cells of half 1 - MA at step t, and rows MA
    // of this wave's tile of dh_rec = dz[rows MA] U^T (the planes hold dz_{t + 1} there for MA = 1, dz_t for MA = 0)
    auto phase = [&](auto MA_, int t) {
      constexpr int MA = decltype(MA_)::value;
      if constexpr (ST) {
        if constexpr (MA == 1) {
          if (t < T1) st.half<1>(zt, rz, Tn, t + 1, nr);
        } else {
          st.half<0>(zt, rz, Tn, t, nr);
        }
      }
      float hv[NG];  // the cells' dh_rec words (rows of half 1 - MA, completed in the previous phase)
#pragma unroll
      for (int k = 0; k < NG; ++k) hv[k] = ht[hr + 16 * (1 - MA) * BH_LR + 4 * k];
      if constexpr (TILE) {
        __builtin_amdgcn_sched_barrier(0);
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        const lds_char* ar = zp + ao + 16 * MA * BS_LZ * 2;
        constexpr int NAF = HFREP_BWDS2_NAF;
        bf16x8 af[NAF][3];
        if constexpr (NAF == 2) {
#pragma unroll
          for (int p = 0; p < 3; ++p) af[0][p] = *reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>(ar + p * BS_PL);
        }
#pragma unroll
        for (int ks = 0; ks < DS_KS; ++ks) {
          const int kr = NAF == 2 ? ks + 1 : ks;  // the k-step whose fragments are read here
          if (kr < DS_KS) {
#pragma unroll
            for (int p = 0; p < 3; ++p)
              af[kr % NAF][p] = *reinterpret_cast<const __attribute__((address_space(3))) bf16x8*>(ar + p * BS_PL + 64 * kr);
          }
          acc = mma_split6(af[ks % NAF], up[ks], acc);
          if (ks < NG) cell(std::integral_constant<int, 1 - MA>{}, ks, hv[ks], t);  // (compile-time)
        }
        // one schedule for the whole phase: per k-step its A fragments, then its 6 MFMAs with 3 VALU slots (the
        // cells' math) after each one; loads and LDS stores of the cells go where they fit
#pragma unroll
        for (int ks = 0; ks < DS_KS; ++ks) {
          __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        // rows 16 MA + 4 g + i, column 16 v + c16
        float* hp = ht + (16 * MA + 4 * g) * BH_LR + 16 * v + c16;
#pragma unroll
        for (int i = 0; i < 4; ++i) hp[i * BH_LR] = acc[i];
      } else {
#pragma unroll
        for (int k = 0; k < NG; ++k) cell(std::integral_constant<int, 1 - MA>{}, k, hv[k], t);
      }
      lds_barrier();
    };
    for (int t = T1; t >= 0; --t) {
      phase(I1{}, t);  // P1(t): B(0, t) + A(1, t)
      phase(I0{}, t);  // P2(t): B(1, t) + A(0, t - 1)
    }
    if constexpr (ST) st.half<1>(zt, rz, Tn, 0, nr);
    __syncthreads();  // (the tiles are re-zeroed for the next row block)
  }
}

template <int ACT, bool HEAD = false>
__global__ void __launch_bounds__(512, 1)
lstmf_bwds2_kernel(const float* __restrict__ dH, const float* __restrict__ tape, const float* __restrict__ U,
                   float* __restrict__ dZ, int B, int Tn, const float* __restrict__ hd, const float* __restrict__ hw) {
  extern __shared__ __attribute__((aligned(16))) float fsm[];
  const int v = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (v < 7) bwds2_run<ACT, HEAD, 3, true, false>(dH, tape, U, dZ, B, Tn, hd, hw, fsm, v);
  else bwds2_run<ACT, HEAD, 4, false, true>(dH, tape, U, dZ, B, Tn, hd, hw, fsm, v);
}

// ==========================================================================================
// host side
// ==========================================================================================
namespace {
template <int KX>
constexpr size_t fwdf_smem() {
  return (size_t)(2 * 32 * FGeo<KX>::LR + 2 * 32 * FGeo<FH>::LR + f_nwl<KX>() * 4 * FNT * 64 + 4) * 4;
}
static_assert(fwdf_smem<100>() <= F_LDS_MAX, "fp32 forward LDS");

template <int KX>
constexpr size_t fwds_smem() {
  return (size_t)(2 * 32 * FGeo<KX>::LR) * 4 + 2 * FS_HB + 16;
}
static_assert(fwds2_smem<32>() <= F_LDS_MAX, "two-wave split forward LDS");
static_assert(fwd2_smem() <= F_LDS_MAX, "eight-wave exact forward LDS");
// forward: 1 exact, 2 the split-recurrent forward for the K <= 36 layers (lstmf_fwds_kernel), 3 the split
// forward on two waves per SIMD where it is instantiated (lstmf_fwds2_kernel, K = 32) and 2 elsewhere
static std::atomic<int>& fwdf_impl() {
  static std::atomic<int> v{fp32_exact() ? 1 : 3};
  return v;
}
static int fwdf_version() { return fwdf_impl().load(std::memory_order_relaxed); }
// the K = 100 forward, under every value of the switch above: 1 the four-wave lstmf_fwd_kernel, 2 the exact
// forward on two waves per SIMD (lstmf_fwd2_kernel; same bits)
static std::atomic<int>& fwdf100_impl() {
  static std::atomic<int> v{2};
  return v;
}
template <int ACT, int KX, bool TAPE, bool TAN>
void fwd2_launch(const float* x, const float* W, const float* b, const float* U, const float* pt, float* hs, float* tp,
                 int B, int Tn, hipStream_t s) {
  const int nrb = (B + 31) / 32, cus = device_cu_count();
  auto k = lstmf_fwd2_kernel<ACT, KX, TAPE, TAN>;
  allow_lds(reinterpret_cast<const void*>(k));
  hipLaunchKernelGGL(k, dim3(nrb < cus ? nrb : cus), dim3(512), fwd2_smem(), s, x, W, b, U, pt, hs, tp, B, Tn);
}
template <int ACT, int KX, bool TAPE, bool TAN, int SKEW>
void fwds2_launch(const float* x, const float* W, const float* b, const float* U, const float* pt, float* hs, float* tp,
                  int B, int Tn, hipStream_t s) {
  const int nrb = (B + 31) / 32, cus = device_cu_count();
  auto k = lstmf_fwds2_kernel<ACT, KX, TAPE, TAN, SKEW>;
  allow_lds(reinterpret_cast<const void*>(k));
  hipLaunchKernelGGL(k, dim3(nrb < cus ? nrb : cus), dim3(512), fwds2_smem<KX>(), s, x, W, b, U, pt, hs, tp, B, Tn);
}
template <int ACT, int KX, bool TAPE, bool TAN>
void fwdf_launch(const float* x, const float* W, const float* b, const float* U, const float* pt, float* hs, float* tp,
                 int B, int Tn, hipStream_t s) {
  const int nrb = (B + 31) / 32, cus = device_cu_count();
  if constexpr (KX == 100) {
    if (fwdf100_impl().load(std::memory_order_relaxed) == 2)
      return fwd2_launch<ACT, KX, TAPE, TAN>(x, W, b, U, pt, hs, tp, B, Tn, s);
  }
  if constexpr (KX == 32) {
    const int ver = fwdf_version();
    if (ver == 3) return fwds2_launch<ACT, KX, TAPE, TAN, HFREP_FWDS2_SKEW>(x, W, b, U, pt, hs, tp, B, Tn, s);
#ifdef HFREP_FWDS2_AB  // A/B builds only: impl 30 + SKEW selects a phase-skew variant (tanh)
    if constexpr (ACT == ACT_TANH) {
      if (ver == 30) return fwds2_launch<ACT, KX, TAPE, TAN, 0>(x, W, b, U, pt, hs, tp, B, Tn, s);
      if (ver == 31) return fwds2_launch<ACT, KX, TAPE, TAN, 1>(x, W, b, U, pt, hs, tp, B, Tn, s);
      if (ver == 32) return fwds2_launch<ACT, KX, TAPE, TAN, 2>(x, W, b, U, pt, hs, tp, B, Tn, s);
      if (ver == 33) return fwds2_launch<ACT, KX, TAPE, TAN, 3>(x, W, b, U, pt, hs, tp, B, Tn, s);
    }
#endif
  }
  // (K = 35 / 36 tangent forwards: the split kernel spills there -- registers; they stay exact)
  if constexpr (FGeo<KX>::KS <= 8 || (FGeo<KX>::KS <= 12 && !TAN)) {
    if (fwdf_version() >= 2) {
      auto k = lstmf_fwds_kernel<ACT, KX, TAPE, TAN>;
      allow_lds(reinterpret_cast<const void*>(k));
      hipLaunchKernelGGL(k, dim3(nrb < cus ? nrb : cus), dim3(256), fwds_smem<KX>(), s, x, W, b, U, pt, hs, tp, B, Tn);
      return;
    }
  }
  auto k = lstmf_fwd_kernel<ACT, KX, TAPE, TAN>;
  allow_lds(reinterpret_cast<const void*>(k));
  hipLaunchKernelGGL(k, dim3(nrb < cus ? nrb : cus), dim3(256), fwdf_smem<KX>(), s, x, W, b, U, pt, hs, tp, B, Tn);
}
template <int KX, bool TAPE, bool TAN>
void fwdf_act(int act, const float* x, const float* W, const float* b, const float* U, const float* pt, float* hs,
              float* tp, int B, int Tn, hipStream_t s) {
  switch (act) {
    case ACT_LINEAR: fwdf_launch<ACT_LINEAR, KX, TAPE, TAN>(x, W, b, U, pt, hs, tp, B, Tn, s); break;
    case ACT_SIGMOID: fwdf_launch<ACT_SIGMOID, KX, TAPE, TAN>(x, W, b, U, pt, hs, tp, B, Tn, s); break;
    default: fwdf_launch<ACT_TANH, KX, TAPE, TAN>(x, W, b, U, pt, hs, tp, B, Tn, s); break;
  }
}
template <bool TAPE, bool TAN>
bool fwdf_k(int K, int act, const float* x, const float* W, const float* b, const float* U, const float* pt, float* hs,
            float* tp, int B, int Tn, hipStream_t s) {
  switch (K) {
    case 32: fwdf_act<32, TAPE, TAN>(act, x, W, b, U, pt, hs, tp, B, Tn, s); return true;
    case 35: fwdf_act<35, TAPE, TAN>(act, x, W, b, U, pt, hs, tp, B, Tn, s); return true;
    case 36: fwdf_act<36, TAPE, TAN>(act, x, W, b, U, pt, hs, tp, B, Tn, s); return true;
    case 100: fwdf_act<100, TAPE, TAN>(act, x, W, b, U, pt, hs, tp, B, Tn, s); return true;
    default: return false;
  }
}
}  // namespace

int set_lstmf_fwd_impl(int v) { return fwdf_impl().exchange(v); }
int set_lstmf_fwd100_impl(int v) { return fwdf100_impl().exchange(v); }

bool lstmf_supported(int H, int K, int act) {
  return H == FH && (K == 32 || K == 35 || K == 36 || K == 100) && (act == ACT_LINEAR || act == ACT_SIGMOID || act == ACT_TANH);
}

bool launch_lstmf_fwd(const float* x, const float* W, const float* b, const float* U, float* hs, float* tape, int B,
                      int Tn, int K, int H, int act, hipStream_t s) {
  if (!lstmf_supported(H, K, act) || B <= 0 || Tn <= 0) return false;
  if (tape) return fwdf_k<true, false>(K, act, x, W, b, U, nullptr, hs, tape, B, Tn, s);
  return fwdf_k<false, false>(K, act, x, W, b, U, nullptr, hs, nullptr, B, Tn, s);
}

bool launch_lstmf_tfwd(const float* xd, const float* W, const float* U, const float* tape, float* hds, float* ttape,
                       int B, int Tn, int K, int H, int act, hipStream_t s) {
  if (!lstmf_supported(H, K, act) || B <= 0 || Tn <= 0) return false;
  return fwdf_k<true, true>(K, act, xd, W, nullptr, U, tape, hds, ttape, B, Tn, s);
}

// BPTT: 2 the exact-fp32 role split (lstmf_bwdp_kernel), 3 the split-recurrent BPTT on four waves
// (lstmf_bwds_kernel, the bitwise reference of 4), 4 the split-recurrent BPTT on two waves per SIMD where it is
// instantiated (lstmf_bwds2_kernel: without the kept h adjoints; same bits) and 3 elsewhere
static std::atomic<int>& bwdf_impl() {
  static std::atomic<int> v{fp32_exact() ? 2 : 4};
  return v;
}
template <int ACT>
void bwdf_launch(const float* dH, const float* tape, const float* U, float* dZ, int B, int Tn, hipStream_t s,
                 const float* hd, const float* hw, float* aH) {
  const int ver = bwdf_impl().load(std::memory_order_relaxed);
  const int nrb = (B + 31) / 32, cus = device_cu_count();
  const size_t sm = (size_t)(32 * BZ_LR + 32 * BH_LR + 4 * BZ_KQ) * 4;
  if (ver == 4 && !aH) {  // (with aH kept: the four-wave kernel below)
    auto go = [&](auto k) {
      allow_lds(reinterpret_cast<const void*>(k));
      hipLaunchKernelGGL(k, dim3(nrb < cus ? nrb : cus), dim3(512), sm + 16 + 3 * BS_PL, s, dH, tape, U, dZ, B, Tn, hd,
                         hw);
    };
    if (hd) go(lstmf_bwds2_kernel<ACT, true>);
    else go(lstmf_bwds2_kernel<ACT, false>);
    return;
  }
  if (ver != 2) {
    auto go = [&](auto k) {
      allow_lds(reinterpret_cast<const void*>(k));
      hipLaunchKernelGGL(k, dim3(nrb < cus ? nrb : cus), dim3(256), sm + 16 + 3 * BS_PL, s, dH, tape, U, dZ, B, Tn, hd,
                         hw, aH);
    };
    if (aH) {
      if (hd) go(lstmf_bwds_kernel<ACT, true, true>);
      else go(lstmf_bwds_kernel<ACT, false, true>);
    } else {
      if (hd) go(lstmf_bwds_kernel<ACT, true>);
      else go(lstmf_bwds_kernel<ACT, false>);
    }
    return;
  }
  if (aH) throw std::runtime_error("lstmf_bwd: the exact-fp32 BPTT does not store the h adjoints (lstmf_ahd_supported)");
  if (hd) throw std::runtime_error("lstmf_bwd: the exact-fp32 BPTT takes a materialised dH (lstmf_head_supported)");
  auto k = lstmf_bwdp_kernel<ACT>;
  allow_lds(reinterpret_cast<const void*>(k));
  hipLaunchKernelGGL(k, dim3(nrb < cus ? nrb : cus), dim3(512), sm, s, dH, tape, U, dZ, B, Tn);
}
static_assert((32 * BZ_LR + 32 * BH_LR + 4 * BZ_KQ) * 4 + 16 + 3 * BS_PL <= F_LDS_MAX, "split BPTT LDS");
int set_lstmf_bwd_impl(int v) { return bwdf_impl().exchange(v); }
bool lstmf_head_supported() { return bwdf_impl().load(std::memory_order_relaxed) != 2; }
bool lstmf_ahd_supported() { return bwdf_impl().load(std::memory_order_relaxed) != 2; }
bool launch_lstmf_bwd(const float* dH, const float* tape, const float* U, float* dZ, int B, int Tn, int H, int act,
                      hipStream_t s, const float* hd, const float* hw, float* aH) {
  if (H != FH || B <= 0 || Tn <= 0) return false;
  switch (act) {
    case ACT_LINEAR: bwdf_launch<ACT_LINEAR>(dH, tape, U, dZ, B, Tn, s, hd, hw, aH); return true;
    case ACT_SIGMOID: bwdf_launch<ACT_SIGMOID>(dH, tape, U, dZ, B, Tn, s, hd, hw, aH); return true;
    case ACT_TANH: bwdf_launch<ACT_TANH>(dH, tape, U, dZ, B, Tn, s, hd, hw, aH); return true;
    default: return false;
  }
}

template <int ACT>
void tbwdf_launch(const float* dH, const float* dHd, const float* tape, const float* ttape, const float* U, float* dZ,
                  float* dZd, int B, int Tn, hipStream_t s, const float* hd, const float* hdd, const float* hw) {
  const int cus = device_cu_count();
  const size_t sm = (size_t)(2 * 32 * BZ_LR + 2 * 32 * BH_LR + 4 * BZ_KQ) * 4;
  const int nrb = (B + 31) / 32;
  auto go = [&](auto k) {
    allow_lds(reinterpret_cast<const void*>(k));
    hipLaunchKernelGGL(k, dim3(nrb < cus ? nrb : cus), dim3(512), sm, s, dH, dHd, tape, ttape, U, dZ, dZd, B, Tn, hd, hdd,
                       hw);
  };
  if (hw) go(lstmf_tbwdp_kernel<ACT, true>);
  else go(lstmf_tbwdp_kernel<ACT, false>);
}
bool launch_lstmf_tbwd(const float* dH, const float* dHd, const float* tape, const float* ttape, const float* U, float* dZ,
                       float* dZd, int B, int Tn, int H, int act, hipStream_t s, const float* hd, const float* hdd,
                       const float* hw) {
  if (H != FH || B <= 0 || Tn <= 0) return false;
  switch (act) {
    case ACT_LINEAR: tbwdf_launch<ACT_LINEAR>(dH, dHd, tape, ttape, U, dZ, dZd, B, Tn, s, hd, hdd, hw); return true;
    case ACT_SIGMOID: tbwdf_launch<ACT_SIGMOID>(dH, dHd, tape, ttape, U, dZ, dZd, B, Tn, s, hd, hdd, hw); return true;
    case ACT_TANH: tbwdf_launch<ACT_TANH>(dH, dHd, tape, ttape, U, dZ, dZd, B, Tn, s, hd, hdd, hw); return true;
    default: return false;
  }
}
template <int ACT>
void tbwd1f_launch(const float* dH, const float* aH, const float* tape, const float* ttape, const float* U, float* dZ,
                   int B, int Tn, hipStream_t s, const float* hd, const float* hw) {
  const int cus = device_cu_count();
  const size_t sm = (size_t)(32 * BZ_LR + 32 * BH_LR + 4 * BZ_KQ) * 4;
  const int nrb = (B + 31) / 32;
  auto go = [&](auto k) {
    allow_lds(reinterpret_cast<const void*>(k));
    hipLaunchKernelGGL(k, dim3(nrb < cus ? nrb : cus), dim3(512), sm, s, dH, aH, tape, ttape, U, dZ, B, Tn, hd, hw);
  };
  if (hw) go(lstmf_tbwd1_kernel<ACT, true>);
  else go(lstmf_tbwd1_kernel<ACT, false>);
}
bool launch_lstmf_tbwd1(const float* dH, const float* aH, const float* tape, const float* ttape, const float* U, float* dZ,
                        int B, int Tn, int H, int act, hipStream_t s, const float* hd, const float* hw) {
  if (H != FH || B <= 0 || Tn <= 0 || !aH) return false;
  switch (act) {
    case ACT_LINEAR: tbwd1f_launch<ACT_LINEAR>(dH, aH, tape, ttape, U, dZ, B, Tn, s, hd, hw); return true;
    case ACT_SIGMOID: tbwd1f_launch<ACT_SIGMOID>(dH, aH, tape, ttape, U, dZ, B, Tn, s, hd, hw); return true;
    case ACT_TANH: tbwd1f_launch<ACT_TANH>(dH, aH, tape, ttape, U, dZ, B, Tn, s, hd, hw); return true;
    default: return false;
  }
}
size_t lstmf_tape_elems(int B, int Tn) { return (size_t)((B + 31) / 32) * Tn * FT_STEP; }

}  // namespace hfrep
