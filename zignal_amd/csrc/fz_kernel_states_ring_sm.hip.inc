// fz_states_ring_sm_kernel -- hand-written gfx950 (MI355X, CDNA4) skeleton of the BLOCK-START STATES of a recording whose graph has
// delay lines deeper than 8 samples, on STREAM-MAJOR buffers (include/flowz_hip.h: fz_run_recording_ring_grad_stream_major).  What it
// computes and stores is fz_kernel_states_ring.hip.inc's -- the T rows of the window forward with the generated fz_adj::fwd in ring mode
// (fz_codegen.cpp: gen_adjoint_body), one lane per stream, the value rings of the deep lines in the lane's LDS column; the state before
// rows 0, B, 2B, ... of the window into starts[ceil(T / B)][n_state][n_streams] in the caller's row order (fz_dump_state, that text's),
// the state after the window's last row into state_out if that is given, nothing else -- so the bits are the time-major kernel's.  How
// x arrives is fz_kernel_states_sm.hip.inc's: in is [n_streams][rows_total][n_in], the recording the window of rows
// [row0, row0 + n_samples); the 64 lanes of a wave fetch a PATCH of [64 streams][FZ_R rows] as float4 pieces laid along the rows, park
// them in a wave-private LDS patch that carries x only, and every lane reads its own row back in groups of FZ_U.
//
// Where the two do not simply paste together (fz_kernel_adjoint_ring_sm.hip.inc has the same points):
//   * LDS is ONE static array: ring[slot][lane], FZ_RING_SLOTS x FZ_BLOCK floats, then the patches [FZ_BLOCK / 64][64 * FZ_AROW]
//     (FZ_BLOCK is whole waves: they start on a 256-byte boundary).  4 FZ_BLOCK (FZ_RING_SLOTS + FZ_R n_in + 4) bytes:
//     fz_grad.cpp: ring_states_sm_geometry chooses FZ_BLOCK and FZ_R together.  A graph without input wires declares no patch;
//   * idle lanes of the last wave shadow the wave's last stream (prow: its patch row, its state and params rows) but own the ring
//     column of their threadIdx.x; they store nothing -- no starts, no state_out -- and every address they form is in bounds.  A wave
//     past the last stream returns whole.  No workgroup barrier, no atomic: fz_wave_sync orders a wave's own patch traffic, a lane's
//     ring column is its own;
//   * a block start (a comparison of two scalars: the row, the next block's first row) may fall anywhere in a patch and anywhere in
//     an unrolled group; a last patch shorter than FZ_R runs the rows it has;
//   * there is no next-group prefetch into registers (xb of the time-major text): the patch is the prefetch.
//
// HBM bytes per stream-sample: 4 n_in + 4 n_state / B, as the time-major text.
//
// Compiled by hiprtc with the build options of every other kernel: -ffp-contract=off (no FMA: one rounding per operation), correctly
// rounded division and square root, denormals kept.
#include "fz_graph_config.h"   // generated: FZ_NIN FZ_NOUT FZ_NCONST FZ_NPARAM FZ_NSTATE FZ_NREG FZ_NRL FZ_NRR FZ_RING_SLOTS FZ_U FZ_R FZ_BLOCK
                               // FZ_KERNEL and the tables fz_reg_row, fz_rl_row0 / fz_rl_depth / fz_rl_slot0, fz_rr_line / fz_rr_delay

#define FZ_P 1
typedef float V;
typedef double VD;
#define FZ_A(n) ((n) > 0 ? (n) : 1)

#include "fz_graph_body.h"     // generated: struct fz_adj { fwd, bwd } in ring mode; fwd is all this kernel calls

#if (FZ_R % 4) != 0 || (FZ_R % FZ_U) != 0 || (FZ_BLOCK % 64) != 0
#error "stream-major ring states: the patch is a multiple of the unrolled group and of 4 rows, the workgroup whole waves"
#endif
#define FZ_AX (FZ_R * FZ_NIN)                 /* floats of x per patch row */
#define FZ_AROW (FZ_AX + 4)                   /* padded patch row */
#define FZ_API (FZ_AX / 4)                    /* float4 pieces per stream and patch */

//@splice fz_kernel_adjoint_patch.hip.inc   (the fetch is all this kernel uses of it)

struct fz_states_ring_sm_args {   // the layout of fz_states_sm_args (fz_kernel_states_sm.hip.inc): one host-side image serves both
   const float* in;            // [n_streams][rows_total][n_in]
   const float* state;         // [n_state][n_streams]   the state before the recording (register and ring lines' rows)
   const float* params;        // [n_param][n_streams]
   float* starts;              // [ceil(T / B)][n_state][n_streams]   the state before rows 0, B, 2B, ... of the window
   float* state_out;           // [n_state][n_streams]   the state after the window's last row; null: not written
   unsigned long long n_streams;
   unsigned int n_samples;     // T >= 1
   unsigned int block_rows;    // B >= 1
   unsigned int rows_total;
   unsigned int row0;
   float c[FZ_A(FZ_NCONST)];   // the program's uniform coefficients
};

// the whole state in the caller's rows: the register rows, then every ring line read back from its value ring, youngest value first
// (fz_kernel_states_ring.hip.inc's)
static __device__ __forceinline__ void fz_dump_state(float* dst, size_t ns, const float* st, const float* ring, const unsigned* pos)
{
#pragma unroll
   for (int r = 0; r < FZ_NREG; ++r) dst[(size_t)fz_reg_row[r] * ns] = st[r];
#pragma unroll
   for (int l = 0; l < FZ_NRL; ++l) {
      const unsigned D = fz_rl_depth[l];
      unsigned slot = pos[l];                              // (the slot of u[t]: the row before it is u[t-1], the state row row0)
#pragma unroll 4
      for (unsigned j = 0; j < D; ++j) {
         slot = slot ? slot - 1u : D - 1u;
         dst[(size_t)(fz_rl_row0[l] + j) * ns] = ring[(size_t)(fz_rl_slot0[l] + slot) * FZ_BLOCK];
      }
   }
}

extern "C" __global__ __launch_bounds__(FZ_BLOCK) void FZ_KERNEL(fz_states_ring_sm_args a)
{
   // ring[slot][lane], then the waves' patches (FZ_RING_SLOTS * FZ_BLOCK floats are whole multiples of 256 bytes)
#if FZ_NIN > 0
   __shared__ __attribute__((aligned(16))) float fz_ring[FZ_RING_SLOTS * FZ_BLOCK + (FZ_BLOCK / 64) * 64 * FZ_AROW];
#else
   __shared__ float fz_ring[FZ_RING_SLOTS * FZ_BLOCK];
#endif
   const size_t ns = a.n_streams;
   const unsigned lane = threadIdx.x & 63u;
   const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (wave-uniform: addresses built from it stay scalar)
   const size_t s_base = (size_t)blockIdx.x * FZ_BLOCK + wave * 64u;                          // first stream of this wave
   if (s_base >= ns) return;                                  // a wave past the last stream (no workgroup barriers below)
   const unsigned rows_here = (unsigned)(ns - s_base < 64u ? ns - s_base : 64u);
   const bool active = lane < rows_here;
   const unsigned prow = active ? lane : rows_here - 1u;      // idle lanes shadow the wave's last stream, store nothing
   const size_t s = s_base + prow;
   float* const ring = fz_ring + threadIdx.x;                 // the lane's OWN column (an idle lane's too): slot q of line l is ring[(fz_rl_slot0[l] + q) * FZ_BLOCK]
   const unsigned T = a.n_samples, B = a.block_rows;
   const unsigned npatch = (T + (unsigned)FZ_R - 1u) / (unsigned)FZ_R;
#if FZ_NIN > 0
   float* const patch = fz_ring + FZ_RING_SLOTS * FZ_BLOCK + wave * (64u * FZ_AROW);
   const float* const mine = patch + prow * FZ_AROW;
   const size_t istride = (size_t)a.rows_total * FZ_NIN;
   const float* const gin = a.in + s_base * istride + (size_t)a.row0 * FZ_NIN;   // the wave's first run: stream s_base, row row0
#endif

   float c[FZ_A(FZ_NCONST)], p[FZ_A(FZ_NPARAM)], st[FZ_A(FZ_NREG)];
   unsigned pos[FZ_NRL];                                      // the row number modulo each ring line's depth (uniform over the wave)
#pragma unroll
   for (int k = 0; k < FZ_NCONST; ++k) c[k] = a.c[k];
#pragma unroll
   for (int k = 0; k < FZ_NPARAM; ++k) p[k] = a.params[(size_t)k * ns + s];
   if (FZ_NCONST == 0) c[0] = 0.f;
   if (FZ_NPARAM == 0) p[0] = 0.f;
   st[0] = 0.f;
#pragma unroll
   for (int r = 0; r < FZ_NREG; ++r) st[r] = a.state[(size_t)fz_reg_row[r] * ns + s];
#pragma unroll
   for (int l = 0; l < FZ_NRL; ++l) {                         // the value rings: slot D - 1 - j holds u[-1-j], the caller's state row row0 + j
      const unsigned D = fz_rl_depth[l];
#pragma unroll 4
      for (unsigned j = 0; j < D; ++j) ring[(size_t)(fz_rl_slot0[l] + D - 1u - j) * FZ_BLOCK] = a.state[(size_t)(fz_rl_row0[l] + j) * ns + s];
      pos[l] = 0u;
   }

   unsigned tn = 0;                                           // the first row of the next block
   float* sk = a.starts + s;                                  // its rows of `starts`
   for (unsigned pk = 0; pk < npatch; ++pk) {
      const unsigned r0 = pk * (unsigned)FZ_R, np = T - r0 < (unsigned)FZ_R ? T - r0 : (unsigned)FZ_R;   // rows of this patch (1 .. FZ_R)
#if FZ_NIN > 0
      fz_wave_sync();                                         // (the rows of the patch before are read)
      fz_patch_fetch<FZ_API>(patch, gin + (size_t)r0 * FZ_NIN, istride, rows_here, np * FZ_NIN, lane);
      fz_wave_sync();
#endif
      for (unsigned j0 = 0; j0 < np; j0 += FZ_U) {
         float x[FZ_U][FZ_A(FZ_NIN)];
#pragma unroll
         for (int j = 0; j < FZ_U; ++j) {                     // (own-row reads inside the patch row: rows behind np hold parked pieces)
            x[j][0] = 0.f;
#if FZ_NIN > 0
#pragma unroll
            for (int w = 0; w < FZ_NIN; ++w) x[j][w] = mine[(j0 + j) * FZ_NIN + w];
#endif
         }
#pragma unroll
         for (int j = 0; j < FZ_U; ++j) {
            const unsigned t = r0 + j0 + j;
            if (j0 + j < np) {
               if (t == tn) {                                 // (scalars both: no lane diverges)
                  if (active) fz_dump_state(sk, ns, st, ring, pos);
                  sk += (size_t)FZ_NSTATE * ns;
                  tn += B;
               }
               float rv[FZ_A(FZ_NRR)], sn[FZ_A(FZ_NREG)], u[FZ_NRL];
               rv[0] = 0.f;
               sn[0] = 0.f;
#pragma unroll
               for (int q = 0; q < FZ_NRR; ++q) {
                  const unsigned l = fz_rr_line[q], d = fz_rr_delay[q], D = fz_rl_depth[l];
                  const unsigned slot = pos[l] >= d ? pos[l] - d : pos[l] + D - d;
                  rv[q] = ring[(size_t)(fz_rl_slot0[l] + slot) * FZ_BLOCK];
               }
               fz_adj::fwd(x[j], c, p, st, rv, sn, u);
#pragma unroll
               for (int l = 0; l < FZ_NRL; ++l) {
                  ring[(size_t)(fz_rl_slot0[l] + pos[l]) * FZ_BLOCK] = u[l];
                  pos[l] = pos[l] + 1u == fz_rl_depth[l] ? 0u : pos[l] + 1u;
               }
#pragma unroll
               for (int r = 0; r < FZ_NREG; ++r) st[r] = sn[r];
            }
         }
      }
   }
   if (a.state_out && active) fz_dump_state(a.state_out + s, ns, st, ring, pos);
}
