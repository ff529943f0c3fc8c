// fz_adjoint_sm_kernel / fz_adjoint_loss_sm_kernel -- hand-written gfx950 (MI355X, CDNA4) skeleton of the ADJOINT of one block on
// STREAM-MAJOR buffers (include/flowz_hip.h: fz_run_block_grad_stream_major), and with FZ_LOSS the same UNDER A SQUARED-ERROR LOSS
// (fz_run_block_loss_grad_stream_major).  The algorithm, the generated body (struct fz_adj: fwd / bwd; FZ_LOSS: out), the rule of the
// loss and the order of every operation are those of fz_kernel_adjoint.hip.inc -- one lane per stream, sweep 1 forward with the state
// before every FZ_C-th row into the workspace [chunk][n_state][n_streams], sweep 2 over the chunks from the last to the first with R,
// pb and cb in registers -- so the bits are the time-major kernel's.  What differs is how the frames move.
//
// Frames: in [n_streams][rows_total][n_in], out_grad [n_streams][rows_total][n_out], in_grad like in; the block is the window of rows
// [row0, row0 + n_samples).  A lane-per-row access would touch one cache line per lane.  So the 64 lanes of a wave fetch a PATCH of
// [64 streams][FZ_R rows] as float4 pieces laid along the rows (consecutive lanes take consecutive pieces of one stream's run), park
// them in a wave-private LDS patch, and every lane reads its own row back (the forward stream-major bodies do the same:
// fz_kernel_sm_common.hip.inc; the mover is fz_kernel_adjoint_patch.hip.inc).  FZ_R is a multiple of FZ_C and of 4 (fz_grad.cpp:
// grad_sm_patch_rows): several checkpoint chunks are served from one patch.  A patch row is [FZ_R x n_in floats of x][FZ_R x n_out floats of dL/dy] + 4 floats of padding (the row
// stride is 4 mod 8 floats where it can be, as FZ_SM_ROW: own-row 16-byte accesses do not collide on banks).  Sweep 1 fills the x
// part only.  In sweep 2 the dL/dx of a row overwrites its x in place once the chunk's frames are in registers, and the x part
// leaves for in_grad as float4 pieces when the patch's chunks are done.
//
// Masking, without a barrier (fz_wave_sync orders a wave's own LDS traffic; a wave past the last stream returns as a whole):
//   * the last wave's missing streams: their lanes shadow the wave's last stream (its patch row, its state) and store nothing;
//     their pieces are not stored;
//   * a last patch shorter than FZ_R: a piece that straddles the window's last float is fetched whole (rows_total * n_wires is a
//     multiple of 4 floats: the piece ends inside the stream's buffer) and stored float by float, pieces behind it are not stored:
//     no row of in_grad outside the window is written;
//   * a last chunk shorter than FZ_C: as in the time-major kernel.
//
// FZ_LOSS: the part of the patch behind x carries the TARGET rows where it carried dL/dy (the patch, FZ_R and the LDS bytes are
// unchanged); per row, sweep 2 forms ybar and the loss from the step's outputs y as the time-major kernel does.  If `out` is asked
// for, y overwrites the row's target in place (every lane its own row, after it read the target) and that part leaves as float4
// pieces when the patch's chunks are done, under the straddling-piece rule of in_grad: no row of `out` outside the window is written.
//
// HBM bytes per stream-sample: 4 (2 n_in + n_out + n_in) + 8 n_state / FZ_C, as the time-major kernel (x twice, dL/dy or the target
// once, dL/dx once, a checkpoint written and read back every FZ_C rows), + 4 n_out when `out` is asked for.
//
// Compiled by hiprtc with the build options of every other kernel: -ffp-contract=off, correctly rounded division and square root,
// denormals kept.
#include "fz_graph_config.h"   // generated: FZ_NIN FZ_NOUT FZ_NCONST FZ_NPARAM FZ_NSTATE FZ_C FZ_R FZ_LOSS FZ_BLOCK FZ_KERNEL

#define FZ_P 1
typedef float V;
typedef double VD;
#define FZ_A(n) ((n) > 0 ? (n) : 1)

#include "fz_graph_body.h"     // generated: struct fz_adj { fwd, bwd; FZ_LOSS: out }

#if (FZ_R % 4) != 0 || (FZ_R % FZ_C) != 0 || (FZ_BLOCK % 64) != 0
#error "stream-major adjoint: the patch is a multiple of the checkpoint stride and of 4 rows, the workgroup whole waves"
#endif
#define FZ_AX (FZ_R * FZ_NIN)                 /* floats of x (then of dL/dx) per patch row */
#define FZ_AY (FZ_R * FZ_NOUT)                /* floats of dL/dy (FZ_LOSS: of the target, then of y) per patch row, behind them */
#define FZ_AROW (FZ_AX + FZ_AY + 4)           /* padded patch row */
#define FZ_API (FZ_AX / 4)                    /* float4 pieces per stream and patch */
#define FZ_APO (FZ_AY / 4)

//@splice fz_kernel_adjoint_patch.hip.inc

struct fz_adj_sm_args {
   const float* in;            // [n_streams][rows_total][n_in]
   const float* state;         // [n_state][n_streams]   the state before the block
   const float* params;        // [n_param][n_streams]
#if FZ_LOSS
   const float* target;        // [n_streams][rows_total][n_out]  what y is compared with
#else
   const float* out_grad;      // [n_streams][rows_total][n_out]
#endif
   const float* state_grad;    // [n_state][n_streams]   dL/d(state after the block); null: zero
   float* in_grad;             // [n_streams][rows_total][n_in]   rows of the window written; null: not computed
   float* state0_grad;         // [n_state][n_streams]   written; null: not computed (may be state_grad)
   float* param_grad;          // [n_param][n_streams]   added to; null: not computed
   float* const_grad;          // [n_const][n_streams]   added to; null: not computed
   float* ckpt;                // [n_chunks][n_state][n_streams] workspace
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

extern "C" __global__ __launch_bounds__(FZ_BLOCK) void FZ_KERNEL(fz_adj_sm_args a)
{
   __shared__ __attribute__((aligned(16))) float fz_apatch[FZ_BLOCK / 64][64 * FZ_AROW];
   const size_t ns = a.n_streams;
   const unsigned lane = threadIdx.x & 63u;
   const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (wave-uniform: addresses built from it stay scalar)
   const size_t s_base = (size_t)blockIdx.x * FZ_BLOCK + wave * 64u;                          // first stream of this wave
   if (s_base >= ns) return;                                  // a wave past the last stream (no workgroup barriers below)
   const unsigned rows_here = (unsigned)(ns - s_base < 64u ? ns - s_base : 64u);
   const bool active = lane < rows_here;
   const unsigned prow = active ? lane : rows_here - 1u;      // idle lanes shadow the wave's last stream, store nothing
   const size_t s = s_base + prow;
   const unsigned T = a.n_samples, nck = a.n_chunks;
   const unsigned npatch = (T + (unsigned)FZ_R - 1u) / (unsigned)FZ_R;
   float* const patch = fz_apatch[wave];
   float* const mine = patch + prow * FZ_AROW;
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

   // ---- sweep 1: forward over the block, the state before every chunk into the workspace
   {
      float st[FZ_A(FZ_NSTATE)];
      st[0] = 0.f;
#pragma unroll
      for (int r = 0; r < FZ_NSTATE; ++r) st[r] = a.state[(size_t)r * nsv + s];
      for (unsigned pk = 0; pk < npatch; ++pk) {
         const unsigned r0 = pk * (unsigned)FZ_R, np = T - r0 < (unsigned)FZ_R ? T - r0 : (unsigned)FZ_R;   // rows of this patch (1 .. FZ_R)
         fz_wave_sync();                                     // (the rows of the patch before are read)
         fz_patch_fetch<FZ_API>(patch, gin + (size_t)r0 * FZ_NIN, istride, rows_here, np * FZ_NIN, lane);
         fz_wave_sync();
         const unsigned nk = (np + (unsigned)FZ_C - 1u) / (unsigned)FZ_C;
         for (unsigned kk = 0; kk < nk; ++kk) {
            const unsigned k = pk * (unsigned)(FZ_R / FZ_C) + kk;
            if (active) {
               float* ck = a.ckpt + (size_t)k * FZ_NSTATE * ns + s;
#pragma unroll
               for (int r = 0; r < FZ_NSTATE; ++r) ck[(size_t)r * ns] = st[r];
            }
            if (k + 1 == nck) break;                          // (the last chunk is re-run by sweep 2 only; chunks before it are whole)
            const float* xr = mine + kk * (unsigned)(FZ_C * FZ_NIN);
#pragma unroll
            for (int j = 0; j < FZ_C; ++j) {
               float x[FZ_A(FZ_NIN)], sn[FZ_A(FZ_NSTATE)];
               x[0] = 0.f;
               sn[0] = 0.f;
#pragma unroll
               for (int w = 0; w < FZ_NIN; ++w) x[w] = xr[j * FZ_NIN + w];
               fz_adj::fwd(x, c, p, st, sn);
#pragma unroll
               for (int r = 0; r < FZ_NSTATE; ++r) st[r] = sn[r];
            }
         }
      }
   }

   // ---- sweep 2: patches from the last to the first, the chunks of a patch from its last to its first
   float R[FZ_A(FZ_NSTATE)], pb[FZ_A(FZ_NPARAM)], cb[FZ_A(FZ_NCONST)];
   R[0] = pb[0] = cb[0] = 0.f;
#pragma unroll
   for (int r = 0; r < FZ_NSTATE; ++r) R[r] = a.state_grad ? a.state_grad[(size_t)r * nsv + s] : 0.f;
#pragma unroll
   for (int k = 0; k < FZ_NPARAM; ++k) pb[k] = a.param_grad ? a.param_grad[(size_t)k * nsv + s] : 0.f;
#pragma unroll
   for (int k = 0; k < FZ_NCONST; ++k) cb[k] = a.const_grad ? a.const_grad[(size_t)k * nsv + s] : 0.f;
#if FZ_LOSS
   float ls = a.loss ? a.loss[s] : 0.f;                      // the stream's loss accumulator, in a register for the whole block
   const float gk = a.grad_scale;
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
         const unsigned t0 = k * (unsigned)FZ_C;
         const unsigned n = T - t0 < (unsigned)FZ_C ? T - t0 : (unsigned)FZ_C;   // rows of this chunk (1 .. FZ_C)
         float S[FZ_C][FZ_A(FZ_NSTATE)], X[FZ_C][FZ_A(FZ_NIN)];
         const float* ck = a.ckpt + (size_t)k * FZ_NSTATE * ns + s;
         float* const xr = mine + kk * (unsigned)(FZ_C * FZ_NIN);                 // the chunk's x rows, then its dL/dx rows
         float* const yr = mine + FZ_AX + kk * (unsigned)(FZ_C * FZ_NOUT);        // its dL/dy rows (FZ_LOSS: its target rows, then its y rows)
#pragma unroll
         for (int j = 0; j < FZ_C; ++j) {
            S[j][0] = 0.f;
            X[j][0] = 0.f;
         }
#pragma unroll
         for (int r = 0; r < FZ_NSTATE; ++r) S[0][r] = ck[(size_t)r * ns];
#pragma unroll
         for (int j = 0; j < FZ_C; ++j)
            if ((unsigned)j < n) {
#pragma unroll
               for (int w = 0; w < FZ_NIN; ++w) X[j][w] = xr[j * FZ_NIN + w];
            }
#pragma unroll
         for (int j = 0; j + 1 < FZ_C; ++j)
            if ((unsigned)j + 1u < n) fz_adj::fwd(X[j], c, p, S[j], S[j + 1]);
         // the saved states and frames are opaque from here on: the compiler must not keep the re-run's node values alive for the
         // backward walk (every node of every step of the chunk in registers) instead of re-evaluating them from these
#pragma unroll
         for (int j = 0; j < FZ_C; ++j) {
#pragma unroll
            for (int r = 0; r < FZ_A(FZ_NSTATE); ++r) asm volatile("" : "+v"(S[j][r]));
#pragma unroll
            for (int w = 0; w < FZ_A(FZ_NIN); ++w) asm volatile("" : "+v"(X[j][w]));
         }
#pragma unroll
         for (int j = FZ_C - 1; j >= 0; --j)
            if ((unsigned)j < n) {
               float yb[FZ_A(FZ_NOUT)], xb[FZ_A(FZ_NIN)];
               yb[0] = 0.f;
#if FZ_LOSS
               float y[FZ_A(FZ_NOUT)];
               y[0] = 0.f;
               fz_adj::out(X[j], c, p, S[j], y);
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
               fz_adj::bwd(X[j], c, p, S[j], yb, xb, R, pb, cb);
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
      for (int r = 0; r < FZ_NSTATE; ++r) a.state0_grad[(size_t)r * nse + s] = R[r];
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
