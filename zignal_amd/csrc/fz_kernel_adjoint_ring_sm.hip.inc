// fz_adjoint_ring_sm_kernel / fz_adjoint_ring_loss_sm_kernel and, with FZ_FAR, fz_adjoint_far_sm_kernel / fz_adjoint_far_loss_sm_kernel --
// hand-written gfx950 (MI355X, CDNA4) skeleton of the ADJOINT of one block whose graph has delay lines deeper than 8 samples (FZ_FAR:
// deeper than 256 as well), on STREAM-MAJOR buffers (include/flowz_hip.h: fz_run_block_ring_grad_stream_major,
// fz_run_block_far_grad_stream_major), and with FZ_LOSS the same UNDER A SQUARED-ERROR LOSS (fz_run_block_ring_loss_grad_stream_major,
// fz_run_block_far_loss_grad_stream_major).  The algorithm, the generated body (fz_codegen.cpp: gen_adjoint_body in ring / far mode:
// struct fz_adj { fwd, bwd; FZ_LOSS: out }), the switch FZ_FAR and what stands under it, both paths of a far line's adjoints in sweep 2
// (FZ_FAR_FAST), the rule of the loss and the order of every operation are those of fz_kernel_adjoint_ring.hip.inc -- one lane per
// stream, sweep 1 with its value rings in LDS, the checkpoints of the register rows and the tape, sweep 2 with the adjoint rings in the
// same LDS and the far lines' adjoint ring in the workspace -- so the bits are the time-major kernel's on the transposed buffers.
// Everything that is [row][n_streams] stays so, one coalesced row per access: state, coefficient and accumulator rows, the
// checkpoints, the tape [T][FZ_NRL + FZ_NFL][n_streams], the adjoint ring [FZ_FAR_SLOTS][n_streams] behind it, the caller's slot and
// phase rows -- the workspace is fz_program_ring_grad_workspace's (fz_program_far_grad_workspace's), whichever layout asks.  How the frames
// move is fz_kernel_adjoint_sm.hip.inc's: the 64 lanes of a wave fetch a PATCH of [64 streams][FZ_R rows] as float4 pieces laid along
// the rows, park them in a wave-private LDS patch and every lane reads its own row back; dL/dx overwrites x in place and leaves as
// float4 pieces when the patch's chunks are done.  FZ_LOSS moves the frames as it does there: the part of the patch behind x carries
// the TARGET rows where it carried dL/dy, and if `out` is asked for, y overwrites the row's target in place and leaves like dL/dx.
//
// Where the two do not simply paste together:
//   * sweep 1 runs EVERY row of the block, the last chunk too (the stream-major kernel stops before it): the tape needs the last
//     chunk's u[t] for reads at delays shorter than a chunk.  FZ_FAR: it takes a far value from the tape row the same lane wrote
//     (program order), or from the caller's slots for t < d; a far read whose row was written before the chunk began (fz_fr_chunked)
//     is requested at the head of its chunk, any other in front of its row;
//   * idle lanes of the last wave shadow the wave's last stream (its patch row, its state, its checkpoint, tape and adjoint-ring rows)
//     but own the LDS ring column of their threadIdx.x; they store nothing -- no tape, no checkpoints, no adjoint-ring rows, no outputs;
//     on the per-row path (FZ_FAR_FAST 0), where the generated bwd() itself loads, adds and stores, an idle lane does not call it --
//     and nothing depends on what they read back (rows another lane wrote, without a fence); every address they form is in bounds.  A
//     wave past the last stream returns whole.  No workgroup barrier, no atomic: fz_wave_sync orders a wave's own patch traffic, a
//     lane's ring column is its own;
//   * LDS is ONE static array: ring[slot][lane] of the LDS ring lines, FZ_RING_SLOTS x FZ_BLOCK floats (none for a far graph without
//     one: the far lines use no LDS), then the patches [FZ_BLOCK / 64][64 * FZ_AROW] (FZ_BLOCK is whole waves: they start on a
//     256-byte boundary).  4 FZ_BLOCK (FZ_RING_SLOTS + FZ_R (n_in + n_out) + 4) bytes: fz_grad.cpp: ring_sm_geometry chooses
//     FZ_BLOCK and FZ_R together -- for a far kernel from half the ring kernel's longest patch: it waits on HBM rows and needs the
//     waves more than the run;
//   * rows [row][n_streams] touched once per launch go through a row stride held per lane (nsv / nse), as in the stream-major kernel;
//   * sweep 2 requests a chunk's ring reads together before the re-run: tape row t - d, or the caller's state for t < d; FZ_FAR: the
//     far values with them, and on the fast path the chunk's rule-2 slots and rule-3 targets; x and dL/dy (FZ_LOSS: the target) come
//     from the patch.
// Masking of a short last patch and a short last chunk: fz_kernel_adjoint_sm.hip.inc's -- no row of in_grad (FZ_LOSS: or of
// out) outside the window is written.
//
// Tape loads and stores are one coalesced row each.  HBM bytes per stream-sample: the time-major kernel's of the same mode
// (+ 4 n_out when `out` is asked for).
//
// Compiled by hiprtc with the build options of every other kernel: -ffp-contract=off, correctly rounded division and square root,
// denormals kept.
#include "fz_graph_config.h"   // generated: the macros and tables of fz_kernel_adjoint_ring.hip.inc in the same mode, and FZ_R

#define FZ_P 1
typedef float V;
typedef double VD;
#define FZ_A(n) ((n) > 0 ? (n) : 1)
#if !FZ_FAR
#define FZ_NFL 0
#define FZ_NFR 0
#endif
#define FZ_NT (FZ_NRL + FZ_NFL)     // tape lines: the ring lines, then the far lines
#define FZ_NRV (FZ_NRR + FZ_NFR)    // values a row reads from the tape: the ring reads, then the far reads

#include "fz_graph_body.h"     // generated: struct fz_adj { fwd, bwd; FZ_LOSS: out }

#if (FZ_R % 4) != 0 || (FZ_R % FZ_C) != 0 || (FZ_BLOCK % 64) != 0
#error "stream-major ring adjoint: the patch is a multiple of the checkpoint stride and of 4 rows, the workgroup whole waves"
#endif
#define FZ_AX (FZ_R * FZ_NIN)                 /* floats of x (then of dL/dx) per patch row */
#define FZ_AY (FZ_R * FZ_NOUT)                /* floats of dL/dy (FZ_LOSS: of the target, then of y) per patch row, behind them */
#define FZ_AROW (FZ_AX + FZ_AY + 4)           /* padded patch row */
#define FZ_API (FZ_AX / 4)                    /* float4 pieces per stream and patch */
#define FZ_APO (FZ_AY / 4)

//@splice fz_kernel_adjoint_patch.hip.inc

struct fz_adj_ring_sm_args {   // the layout of fz_adj_sm_args (fz_kernel_adjoint_sm.hip.inc): one host-side image serves the family, both modes
   const float* in;            // [n_streams][rows_total][n_in]
   const float* state;         // [n_state][n_streams]   the state before the block (register rows, ring rows, far slots, phase rows)
   const float* params;        // [n_param][n_streams]
#if FZ_LOSS
   const float* target;        // [n_streams][rows_total][n_out]  what y is compared with
#else
   const float* out_grad;      // [n_streams][rows_total][n_out]
#endif
   const float* state_grad;    // [n_state][n_streams]   dL/d(state after the block); null: zero.  A far line's phase row is never read
   float* in_grad;             // [n_streams][rows_total][n_in]   rows of the window written; null: not computed
   float* state0_grad;         // [n_state][n_streams]   written; null: not computed (may be state_grad)
   float* param_grad;          // [n_param][n_streams]   added to; null: not computed
   float* const_grad;          // [n_const][n_streams]   added to; null: not computed
   float* ckpt;                // the workspace: [n_chunks][FZ_NREG][n_streams] checkpoints, [T][FZ_NT][n_streams] the tape, FZ_FAR: the adjoint ring
#if FZ_LOSS
   float* loss;                // [n_streams]            the sum of e * e, added to; null: not computed
   float* out;                 // [n_streams][rows_total][n_out]  y, rows of the window written; null: not written
#endif
   unsigned long long n_streams;
   unsigned int n_samples;
   unsigned int n_chunks;      // ceil(n_samples / FZ_C)
#if FZ_LOSS
   float grad_scale;           // ybar = (y - target) * grad_scale
#endif
   unsigned int rows_total;
   unsigned int row0;
   float c[FZ_A(FZ_NCONST)];   // the program's uniform coefficients
};

#if FZ_FAR
//@splice fz_kernel_far.hip.inc
typedef size_t fz_row_t;       // a row number of the block (t0, t): 64 bits where fz_far_value takes it,
#else
typedef unsigned fz_row_t;     // 32 where the ring kernel alone indexes the tape with it -- the width each mode's machine code was made with
#endif

extern "C" __global__ __launch_bounds__(FZ_BLOCK) void FZ_KERNEL(fz_adj_ring_sm_args a)
{
   // ring[slot][lane] of the LDS ring lines, then the waves' patches (FZ_RING_SLOTS * FZ_BLOCK floats are whole multiples of 256 bytes)
   __shared__ __attribute__((aligned(16))) float fz_ring[FZ_RING_SLOTS * FZ_BLOCK + (FZ_BLOCK / 64) * 64 * FZ_AROW];
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
   const unsigned T = a.n_samples, nck = a.n_chunks;
   const unsigned npatch = (T + (unsigned)FZ_R - 1u) / (unsigned)FZ_R;
   float* const patch = fz_ring + FZ_RING_SLOTS * FZ_BLOCK + wave * (64u * FZ_AROW);
   float* const mine = patch + prow * FZ_AROW;
   float* const tape = a.ckpt + (size_t)nck * FZ_NREG * ns + s;
#if FZ_FAR
   float* const fa = tape + (size_t)T * FZ_NT * ns;           // the lane's column of the adjoint ring: row k is fa[k * ns]
   const float* const state = a.state + s;                    // the lane's column of the caller's state, for the far lines' rows
#endif
   // the wave's first run of each buffer: stream s_base, row row0
   const size_t istride = (size_t)a.rows_total * FZ_NIN, ostride = (size_t)a.rows_total * FZ_NOUT;
   const float* const gin = FZ_NIN ? a.in + s_base * istride + (size_t)a.row0 * FZ_NIN : nullptr;
#if FZ_LOSS
   const float* const gyb = FZ_NOUT ? a.target + s_base * ostride + (size_t)a.row0 * FZ_NOUT : nullptr;
   float* const gyo = FZ_NOUT && a.out ? a.out + s_base * ostride + (size_t)a.row0 * FZ_NOUT : nullptr;
#else
   const float* const gyb = FZ_NOUT ? a.out_grad + s_base * ostride + (size_t)a.row0 * FZ_NOUT : nullptr;
#endif
   float* const gxb = FZ_NIN && a.in_grad ? a.in_grad + s_base * istride + (size_t)a.row0 * FZ_NIN : nullptr;

   // (rows [row][n_streams] that are touched once per launch go through a row stride held per lane: as a scalar, every multiple of it
   //  -- one per parameter and accumulator row -- would stay in scalar registers from here to the epilogue)
   size_t nsv = ns;
   asm volatile("" : "+v"(nsv));
   float c[FZ_A(FZ_NCONST)], p[FZ_A(FZ_NPARAM)];
#pragma unroll
   for (int k = 0; k < FZ_NCONST; ++k) c[k] = a.c[k];
#pragma unroll
   for (int k = 0; k < FZ_NPARAM; ++k) p[k] = a.params[(size_t)k * nsv + s];
   if (FZ_NCONST == 0) c[0] = 0.f;
   if (FZ_NPARAM == 0) p[0] = 0.f;
#if FZ_FAR
   unsigned fp0[FZ_A(FZ_NFL)];                                // the far lines' phases before the block, modulo their depths
   fp0[0] = 0u;
#pragma unroll
   for (int f = 0; f < FZ_NFL; ++f)
      fp0[f] = __builtin_amdgcn_readfirstlane((unsigned)state[(size_t)fz_fl_phase_row[f] * nsv]) % fz_fl_depth[f];
#endif

   // ---- sweep 1: forward over EVERY row of the block; the register rows before every chunk and every row's ring- and far-line values into the workspace
   {
      float st[FZ_A(FZ_NREG)];
      unsigned pos[FZ_A(FZ_NRL)];                          // the row number modulo each ring line's depth (uniform over the wave)
      st[0] = 0.f;
      pos[0] = 0u;
#pragma unroll
      for (int r = 0; r < FZ_NREG; ++r) st[r] = a.state[(size_t)fz_reg_row[r] * nsv + s];
#pragma unroll
      for (int l = 0; l < FZ_NRL; ++l) {                   // the value rings: slot D - 1 - j holds u[-1-j], the caller's state row row0 + j
         const unsigned D = fz_rl_depth[l];
#pragma unroll 4
         for (unsigned j = 0; j < D; ++j) ring[(size_t)(fz_rl_slot0[l] + D - 1u - j) * FZ_BLOCK] = a.state[(size_t)(fz_rl_row0[l] + j) * nsv + s];
         pos[l] = 0u;
      }
      for (unsigned pk = 0; pk < npatch; ++pk) {
         const unsigned r0 = pk * (unsigned)FZ_R, np = T - r0 < (unsigned)FZ_R ? T - r0 : (unsigned)FZ_R;   // rows of this patch (1 .. FZ_R)
         fz_wave_sync();                                     // (the rows of the patch before are read)
         fz_patch_fetch<FZ_API>(patch, gin + (size_t)r0 * FZ_NIN, istride, rows_here, np * FZ_NIN, lane);
         fz_wave_sync();
         const unsigned nk = (np + (unsigned)FZ_C - 1u) / (unsigned)FZ_C;
         for (unsigned kk = 0; kk < nk; ++kk) {
            const unsigned k = pk * (unsigned)(FZ_R / FZ_C) + kk;
            const fz_row_t t0 = (fz_row_t)k * FZ_C;
            const unsigned n = T - (unsigned)t0 < (unsigned)FZ_C ? T - (unsigned)t0 : (unsigned)FZ_C;   // rows of this chunk (1 .. FZ_C)
            if (active) {
               float* ck = a.ckpt + (size_t)k * FZ_NREG * ns + s;
#pragma unroll
               for (int r = 0; r < FZ_NREG; ++r) ck[(size_t)r * ns] = st[r];
            }
            const float* xr = mine + kk * (unsigned)(FZ_C * FZ_NIN);
#if FZ_FAR
            float FV[FZ_C][FZ_A(FZ_NFR)];
            // the far reads whose rows were written before the chunk began, requested together
#pragma unroll
            for (int j = 0; j < FZ_C; ++j) {
               FV[j][0] = 0.f;
               if ((unsigned)j < n) {
#pragma unroll
                  for (int q = 0; q < FZ_NFR; ++q)
                     if (fz_fr_chunked[q]) FV[j][q] = fz_far_value(tape, state, ns, fp0, q, t0 + j);
               }
            }
#endif
#pragma unroll
            for (int j = 0; j < FZ_C; ++j)
               if ((unsigned)j < n) {
                  float x[FZ_A(FZ_NIN)], rv[FZ_A(FZ_NRV)], sn[FZ_A(FZ_NREG)], u[FZ_A(FZ_NT)];
                  x[0] = 0.f;
                  rv[0] = 0.f;
                  sn[0] = 0.f;
#pragma unroll
                  for (int w = 0; w < FZ_NIN; ++w) x[w] = xr[j * FZ_NIN + w];
#pragma unroll
                  for (int q = 0; q < FZ_NRR; ++q) {
                     const unsigned l = fz_rr_line[q], d = fz_rr_delay[q], D = fz_rl_depth[l];
                     const unsigned slot = pos[l] >= d ? pos[l] - d : pos[l] + D - d;
                     rv[q] = ring[(size_t)(fz_rl_slot0[l] + slot) * FZ_BLOCK];
                  }
#if FZ_FAR
#pragma unroll
                  for (int q = 0; q < FZ_NFR; ++q)            // (a row of this chunk: the tape row this lane wrote a few rows ago)
                     rv[FZ_NRR + q] = fz_fr_chunked[q] ? FV[j][q] : fz_far_value(tape, state, ns, fp0, q, t0 + j);
#endif
                  fz_adj::fwd(x, c, p, st, rv, sn, u);
#pragma unroll
                  for (int l = 0; l < FZ_NRL; ++l) {
                     ring[(size_t)(fz_rl_slot0[l] + pos[l]) * FZ_BLOCK] = u[l];
#if !FZ_FAR
                     if (active) tape[((size_t)(t0 + j) * FZ_NT + l) * ns] = u[l];
#endif
                     pos[l] = pos[l] + 1u == fz_rl_depth[l] ? 0u : pos[l] + 1u;
                  }
#if FZ_FAR
                  if (active) {
#pragma unroll
                     for (int l = 0; l < FZ_NT; ++l) tape[((t0 + j) * FZ_NT + l) * ns] = u[l];   // (the ring lines' values, then the far lines')
                  }
#endif
#pragma unroll
                  for (int r = 0; r < FZ_NREG; ++r) st[r] = sn[r];
               }
         }
      }
   }

   // ---- sweep 2: patches from the last to the first, the chunks of a patch from its last to its first
   float R[FZ_A(FZ_NREG)], pb[FZ_A(FZ_NPARAM)], cb[FZ_A(FZ_NCONST)];
   R[0] = pb[0] = cb[0] = 0.f;
#pragma unroll
   for (int r = 0; r < FZ_NREG; ++r) R[r] = a.state_grad ? a.state_grad[(size_t)fz_reg_row[r] * nsv + s] : 0.f;
#pragma unroll
   for (int k = 0; k < FZ_NPARAM; ++k) pb[k] = a.param_grad ? a.param_grad[(size_t)k * nsv + s] : 0.f;
#pragma unroll
   for (int k = 0; k < FZ_NCONST; ++k) cb[k] = a.const_grad ? a.const_grad[(size_t)k * nsv + s] : 0.f;
#if FZ_LOSS
   float ls = a.loss ? a.loss[s] : 0.f;                      // the stream's loss accumulator, in a register for the whole block
   const float gk = a.grad_scale;
#endif
#pragma unroll
   for (int l = 0; l < FZ_NRL; ++l) {                      // the adjoint rings in LDS: the slot of u[T-1-j] holds state_grad[row0 + j], or +0.0f
      const unsigned D = fz_rl_depth[l], top = (T - 1u) % D;
#pragma unroll 4
      for (unsigned j = 0; j < D; ++j) {
         const unsigned slot = top >= j ? top - j : top + D - j;
         ring[(size_t)(fz_rl_slot0[l] + slot) * FZ_BLOCK] = a.state_grad ? a.state_grad[(size_t)(fz_rl_row0[l] + j) * nsv + s] : 0.f;
      }
   }
#if FZ_FAR
   if (active) {
#pragma unroll
      for (int f = 0; f < FZ_NFL; ++f) {                   // the adjoint ring in the workspace: slot k holds state_grad[row0 + k], or +0.0f
         const unsigned D = fz_fl_depth[f];
#pragma unroll 4
         for (unsigned k = 0; k < D; ++k)
            fa[(size_t)(fz_fl_slot0[f] + k) * nsv] = a.state_grad ? a.state_grad[(size_t)(fz_fl_row0[f] + k) * nsv + s] : 0.f;
      }
   }
#endif
   for (unsigned pk = npatch; pk-- > 0;) {
      const unsigned r0 = pk * (unsigned)FZ_R, np = T - r0 < (unsigned)FZ_R ? T - r0 : (unsigned)FZ_R;
      fz_wave_sync();                                        // (the patch before has left for in_grad and out)
      fz_patch_fetch<FZ_API>(patch, gin + (size_t)r0 * FZ_NIN, istride, rows_here, np * FZ_NIN, lane);
      fz_patch_fetch<FZ_APO>(patch + FZ_AX, gyb + (size_t)r0 * FZ_NOUT, ostride, rows_here, np * FZ_NOUT, lane);
      fz_wave_sync();
      const unsigned nk = (np + (unsigned)FZ_C - 1u) / (unsigned)FZ_C;
      for (unsigned kk = nk; kk-- > 0;) {
         const unsigned k = pk * (unsigned)(FZ_R / FZ_C) + kk;
         const fz_row_t t0 = (fz_row_t)k * FZ_C;
         const unsigned n = T - (unsigned)t0 < (unsigned)FZ_C ? T - (unsigned)t0 : (unsigned)FZ_C;   // rows of this chunk (1 .. FZ_C)
         float S[FZ_C][FZ_A(FZ_NREG)], X[FZ_C][FZ_A(FZ_NIN)], RV[FZ_C][FZ_A(FZ_NRV)];
         const float* ck = a.ckpt + (size_t)k * FZ_NREG * ns + s;
         float* const xr = mine + kk * (unsigned)(FZ_C * FZ_NIN);                 // the chunk's x rows, then its dL/dx rows
         float* const yr = mine + FZ_AX + kk * (unsigned)(FZ_C * FZ_NOUT);        // its dL/dy rows (FZ_LOSS: its target rows, then its y rows)
#if FZ_FAR
         unsigned fbase[FZ_A(FZ_NFL)];                        // per far line: the slot of row t0
         fbase[0] = 0u;
#pragma unroll
         for (int f = 0; f < FZ_NFL; ++f) fbase[f] = (fp0[f] + (unsigned)(t0 % fz_fl_depth[f])) % fz_fl_depth[f];
#if FZ_FAR_FAST
         float F2[FZ_C][FZ_A(FZ_NFL)], FQ[FZ_C][FZ_A(FZ_NFR)];
#endif
#endif
#pragma unroll
         for (int j = 0; j < FZ_C; ++j) {
            S[j][0] = 0.f;
            X[j][0] = 0.f;
            RV[j][0] = 0.f;
#if FZ_FAR_FAST
            F2[j][0] = 0.f;
            FQ[j][0] = 0.f;
#endif
         }
#pragma unroll
         for (int r = 0; r < FZ_NREG; ++r) S[0][r] = ck[(size_t)r * ns];
         // every ring and far read of the chunk, requested together: tape row t - d, or the caller's state for t < d; on the fast path
         // the chunk's slots of the adjoint ring as well; the frames from the patch
#pragma unroll
         for (int j = 0; j < FZ_C; ++j)
            if ((unsigned)j < n) {
               const fz_row_t t = t0 + j;
#pragma unroll
               for (int q = 0; q < FZ_NRR; ++q) {
                  const unsigned l = fz_rr_line[q], d = fz_rr_delay[q];
                  RV[j][q] = t >= d ? tape[((size_t)(t - d) * FZ_NT + l) * ns] : a.state[(size_t)(fz_rl_row0[l] + d - 1u - (unsigned)t) * ns + s];
               }
#if FZ_FAR
#pragma unroll
               for (int q = 0; q < FZ_NFR; ++q) RV[j][FZ_NRR + q] = fz_far_value(tape, state, ns, fp0, q, t);
#if FZ_FAR_FAST
#pragma unroll
               for (int f = 0; f < FZ_NFL; ++f) F2[j][f] = fa[(size_t)(fz_fl_slot0[f] + fz_far_on(fbase[f], (unsigned)j, fz_fl_depth[f])) * ns];
#pragma unroll
               for (int q = 0; q < FZ_NFR; ++q) {
                  const unsigned f = fz_fr_line[q], d = fz_fr_delay[q], D = fz_fl_depth[f];
                  FQ[j][q] = d == D ? -0.0f : fa[(size_t)(fz_fl_slot0[f] + fz_far_back(fz_far_on(fbase[f], (unsigned)j, D), d, D)) * ns];   // (the full depth: the slot just reset)
               }
#endif
#endif
#pragma unroll
               for (int w = 0; w < FZ_NIN; ++w) X[j][w] = xr[j * FZ_NIN + w];
            }
#pragma unroll
         for (int j = 0; j + 1 < FZ_C; ++j)
            if ((unsigned)j + 1u < n) {
               float u[FZ_A(FZ_NT)];
               fz_adj::fwd(X[j], c, p, S[j], RV[j], S[j + 1], u);
            }
         // the saved states, frames and tape values are opaque from here on: the compiler must not keep the re-run's node values alive
         // for the backward walk instead of re-evaluating them from these
#pragma unroll
         for (int j = 0; j < FZ_C; ++j) {
#pragma unroll
            for (int r = 0; r < FZ_A(FZ_NREG); ++r) asm volatile("" : "+v"(S[j][r]));
#pragma unroll
            for (int w = 0; w < FZ_A(FZ_NIN); ++w) asm volatile("" : "+v"(X[j][w]));
#pragma unroll
            for (int q = 0; q < FZ_A(FZ_NRV); ++q) asm volatile("" : "+v"(RV[j][q]));
         }
         unsigned base[FZ_A(FZ_NRL)];
         base[0] = 0u;
#pragma unroll
         for (int l = 0; l < FZ_NRL; ++l) base[l] = (unsigned)t0 % fz_rl_depth[l];
#pragma unroll
         for (int j = FZ_C - 1; j >= 0; --j)
            if ((unsigned)j < n) {
               float yb[FZ_A(FZ_NOUT)], xb[FZ_A(FZ_NIN)];
               unsigned pt[FZ_A(FZ_NRL)], fpt[FZ_A(FZ_NFL)];   // per ring line: the row number modulo its depth; per far line: the slot of the row
               yb[0] = 0.f;
               xb[0] = 0.f;
               pt[0] = fpt[0] = 0u;
#pragma unroll
               for (int l = 0; l < FZ_NRL; ++l) pt[l] = (base[l] + (unsigned)j) % fz_rl_depth[l];
#if FZ_FAR
#pragma unroll
               for (int f = 0; f < FZ_NFL; ++f) fpt[f] = fz_far_on(fbase[f], (unsigned)j, fz_fl_depth[f]);
#endif
#if FZ_LOSS
               float y[FZ_A(FZ_NOUT)];
               y[0] = 0.f;
               fz_adj::out(X[j], c, p, S[j], RV[j], y);
#pragma unroll
               for (int w = 0; w < FZ_NOUT; ++w) {         // the rule: slots in ascending order, one rounding per operation
                  const float e = y[w] - yr[j * FZ_NOUT + w];
                  yb[w] = e * gk;
                  ls = ls + e * e;
               }
               if (gyo && active) {                          // (the row's target is read: its y takes its place)
#pragma unroll
                  for (int w = 0; w < FZ_NOUT; ++w) yr[j * FZ_NOUT + w] = y[w];
               }
#else
#pragma unroll
               for (int w = 0; w < FZ_NOUT; ++w) yb[w] = yr[j * FZ_NOUT + w];
#endif
#if !FZ_FAR
               fz_adj::bwd(X[j], c, p, S[j], RV[j], yb, xb, R, pb, cb, ring, pt);
#elif FZ_FAR_FAST
               fz_adj::bwd(X[j], c, p, S[j], RV[j], yb, xb, R, pb, cb, ring, pt, F2[j], FQ[j]);
               // the row's slots leave once: rule 2's reset, then what rule 3 made of its targets.  A read at the full depth targets the
               // slot its row just reset -- and a line's depth is its deepest read, so there is one unless the graph was lowered otherwise:
               // then the reset itself never leaves
               if (active) {
#pragma unroll
                  for (int f = 0; f < FZ_NFL; ++f) {
                     bool full = false;
#pragma unroll
                     for (int q = 0; q < FZ_NFR; ++q) full = full || (fz_fr_line[q] == (unsigned)f && fz_fr_delay[q] == fz_fl_depth[f]);
                     if (!full) fa[(size_t)(fz_fl_slot0[f] + fpt[f]) * ns] = -0.0f;
                  }
#pragma unroll
                  for (int q = 0; q < FZ_NFR; ++q) {
                     const unsigned f = fz_fr_line[q];
                     fa[(size_t)(fz_fl_slot0[f] + fz_far_back(fpt[f], fz_fr_delay[q], fz_fl_depth[f])) * ns] = FQ[j][q];
                  }
               }
#else
               // (the per-row path: bwd() loads, adds and stores the adjoint ring's slots itself, so an idle lane stays out of it)
               if (active) fz_adj::bwd(X[j], c, p, S[j], RV[j], yb, xb, R, pb, cb, ring, pt, fa, fpt, ns);
#endif
               if (gxb && active) {                          // (the row's x is in X[j]: its dL/dx takes its place)
#pragma unroll
                  for (int w = 0; w < FZ_NIN; ++w) xr[j * FZ_NIN + w] = xb[w];
               }
            }
      }
#if FZ_LOSS
      if (gxb || gyo) fz_wave_sync();
      if (gxb) fz_patch_flush<FZ_API>(patch, gxb + (size_t)r0 * FZ_NIN, istride, rows_here, np * FZ_NIN, lane);
      if (gyo) fz_patch_flush<FZ_APO>(patch + FZ_AX, gyo + (size_t)r0 * FZ_NOUT, ostride, rows_here, np * FZ_NOUT, lane);
#else
      if (gxb) {
         fz_wave_sync();
         fz_patch_flush<FZ_API>(patch, gxb + (size_t)r0 * FZ_NIN, istride, rows_here, np * FZ_NIN, lane);
      }
#endif
   }
   if (!active) return;
   size_t nse = ns;
   asm volatile("" : "+v"(nse));
   if (a.state0_grad) {
#pragma unroll
      for (int r = 0; r < FZ_NREG; ++r) a.state0_grad[(size_t)fz_reg_row[r] * nse + s] = R[r];
#pragma unroll
      for (int l = 0; l < FZ_NRL; ++l) {                   // after row 0 the slot of u[-1-j] is D - 1 - j
         const unsigned D = fz_rl_depth[l];
#pragma unroll 4
         for (unsigned j = 0; j < D; ++j) a.state0_grad[(size_t)(fz_rl_row0[l] + j) * nse + s] = ring[(size_t)(fz_rl_slot0[l] + D - 1u - j) * FZ_BLOCK];
      }
#if FZ_FAR
#pragma unroll
      for (int f = 0; f < FZ_NFL; ++f) {                   // the far lines: slot k as it is, the phase row +0.0f
         const unsigned D = fz_fl_depth[f];
#pragma unroll 4
         for (unsigned k = 0; k < D; ++k) a.state0_grad[(size_t)(fz_fl_row0[f] + k) * nse + s] = fa[(size_t)(fz_fl_slot0[f] + k) * nse];
         a.state0_grad[(size_t)fz_fl_phase_row[f] * nse + s] = 0.f;
      }
#endif
   }
   if (a.param_grad) {
#pragma unroll
      for (int k = 0; k < FZ_NPARAM; ++k) a.param_grad[(size_t)k * nse + s] = pb[k];
   }
   if (a.const_grad) {
#pragma unroll
      for (int k = 0; k < FZ_NCONST; ++k) a.const_grad[(size_t)k * nse + s] = cb[k];
   }
#if FZ_LOSS
   if (a.loss) a.loss[s] = ls;
#endif
}
