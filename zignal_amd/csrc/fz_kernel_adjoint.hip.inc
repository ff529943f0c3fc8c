// fz_adjoint_kernel / fz_adjoint_loss_kernel -- hand-written gfx950 (MI355X, CDNA4) skeleton of the ADJOINT of one block: reverse-mode
// gradients of fz_run_block (include/flowz_hip.h: fz_run_block_grad), and with FZ_LOSS the same UNDER A SQUARED-ERROR LOSS
// (fz_run_block_loss_grad): dL/dy formed in the kernel instead of read.
//
// One lane owns one stream for the whole block (wave64; the workgroups of the last wave are masked by the stream count).
// The generated body (fz_codegen.cpp: gen_adjoint_body) gives struct fz_adj with
//   fwd(x, c, p, s, sn)                       the state after one step, from the state before it and the step's frame;
//   bwd(x, c, p, s, yb, xb, R, pb, cb)        that step re-evaluated from (s, x), then its adjoint statements in reverse node order;
//   out(x, c, p, s, y)                        FZ_LOSS only: the step's output values.
// Time-major frames [t][stream][wire]; state, parameter and coefficient rows [row][stream].
//
// Sweep 1 runs the block forward without writing an output and stores the state before every FZ_C-th row into the workspace,
// [ceil(T / FZ_C)][n_state][n_streams] (one coalesced row per state float).  Sweep 2 takes the chunks from the last to the first:
// it loads the chunk's checkpoint, re-runs the chunk forward keeping every step's state and frame in registers (fully unrolled:
// constant indices only), then walks the chunk backwards -- the dL/dy row in, bwd(), the dL/dx row out.  The pending line adjoints
// R, the parameter and the coefficient accumulators stay in registers for the whole block.
//
// FZ_LOSS: where the plain kernel reads a dL/dy row, the loss kernel reads the TARGET row and applies the rule of the header, per
// output slot j in ascending order:  e = y[j] - target[t][j];  ybar[j] = e * grad_scale;  loss = loss + e * e  (each operation rounded
// once, no FMA).  ybar then enters bwd() as the dL/dy row does, so every gradient bit is fz_run_block_grad's for that ybar.  The loss
// accumulator is one register per lane for the whole block, next to pb / cb: it starts from the caller's loss[stream] and runs over
// the rows T-1 .. 0 as they do, so blocks chain bitwise.  y leaves for `out` on the way if asked (the bits of fz_run_block).
//
// HBM bytes per stream-sample: 4 (2 n_in + n_out + n_in) + 8 n_state / FZ_C (x twice, dL/dy or the target once, dL/dx once, a
// checkpoint written and read back every FZ_C rows), + 4 n_out when `out` is asked for.
//
// Compiled by hiprtc with the build options of the forward kernels: -ffp-contract=off (no FMA: one rounding per operation),
// correctly rounded division and square root, denormals kept.
#include "fz_graph_config.h"   // generated: FZ_NIN FZ_NOUT FZ_NCONST FZ_NPARAM FZ_NSTATE FZ_C FZ_LOSS FZ_BLOCK FZ_KERNEL

#define FZ_P 1
typedef float V;
typedef double VD;
#define FZ_A(n) ((n) > 0 ? (n) : 1)

#include "fz_graph_body.h"     // generated: struct fz_adj { fwd, bwd; FZ_LOSS: out }

struct fz_adj_args {
   const float* in;            // [T][n_streams][n_in]
   const float* state;         // [n_state][n_streams]   the state before the block
   const float* params;        // [n_param][n_streams]
#if FZ_LOSS
   const float* target;        // [T][n_streams][n_out]  what y is compared with
#else
   const float* out_grad;      // [T][n_streams][n_out]
#endif
   const float* state_grad;    // [n_state][n_streams]   dL/d(state after the block); null: zero
   float* in_grad;             // [T][n_streams][n_in]   written; null: not computed
   float* state0_grad;         // [n_state][n_streams]   written; null: not computed (may be state_grad)
   float* param_grad;          // [n_param][n_streams]   added to; null: not computed
   float* const_grad;          // [n_const][n_streams]   added to; null: not computed
   float* ckpt;                // [n_chunks][n_state][n_streams] workspace
#if FZ_LOSS
   float* loss;                // [n_streams]            the sum of e * e, added to; null: not computed
   float* out;                 // [T][n_streams][n_out]  y, written; null: not written
#endif
   unsigned long long n_streams;
   unsigned int n_samples;
   unsigned int n_chunks;      // ceil(n_samples / FZ_C)
#if FZ_LOSS
   float grad_scale;           // ybar = (y - target) * grad_scale
#endif
   float c[FZ_A(FZ_NCONST)];   // the program's uniform coefficients
};

extern "C" __global__ __launch_bounds__(FZ_BLOCK) void FZ_KERNEL(fz_adj_args a)
{
   const size_t ns = a.n_streams;
   const size_t s = (size_t)blockIdx.x * FZ_BLOCK + threadIdx.x;
   if (s >= ns) return;                                  // the masked tail of the last wave (no barriers below)
   const unsigned T = a.n_samples, nck = a.n_chunks;
   float c[FZ_A(FZ_NCONST)], p[FZ_A(FZ_NPARAM)];
#pragma unroll
   for (int k = 0; k < FZ_NCONST; ++k) c[k] = a.c[k];
#pragma unroll
   for (int k = 0; k < FZ_NPARAM; ++k) p[k] = a.params[(size_t)k * ns + s];
   if (FZ_NCONST == 0) c[0] = 0.f;
   if (FZ_NPARAM == 0) p[0] = 0.f;

   // ---- sweep 1: forward over the block, the state before every chunk into the workspace
   {
      float st[FZ_A(FZ_NSTATE)];
      st[0] = 0.f;
#pragma unroll
      for (int r = 0; r < FZ_NSTATE; ++r) st[r] = a.state[(size_t)r * ns + s];
      for (unsigned k = 0; k < nck; ++k) {
         float* ck = a.ckpt + (size_t)k * FZ_NSTATE * ns + s;
#pragma unroll
         for (int r = 0; r < FZ_NSTATE; ++r) ck[(size_t)r * ns] = st[r];
         if (k + 1 == nck) break;                          // (the last chunk is re-run by sweep 2 only; chunks before it are whole)
         const size_t t0 = (size_t)k * FZ_C;
#pragma unroll
         for (int j = 0; j < FZ_C; ++j) {
            float x[FZ_A(FZ_NIN)], sn[FZ_A(FZ_NSTATE)];
            x[0] = 0.f;
            sn[0] = 0.f;
#pragma unroll
            for (int w = 0; w < FZ_NIN; ++w) x[w] = a.in[((t0 + j) * ns + s) * FZ_NIN + w];
            fz_adj::fwd(x, c, p, st, sn);
#pragma unroll
            for (int r = 0; r < FZ_NSTATE; ++r) st[r] = sn[r];
         }
      }
   }

   // ---- sweep 2: chunks from the last to the first
   float R[FZ_A(FZ_NSTATE)], pb[FZ_A(FZ_NPARAM)], cb[FZ_A(FZ_NCONST)];
   R[0] = pb[0] = cb[0] = 0.f;
#pragma unroll
   for (int r = 0; r < FZ_NSTATE; ++r) R[r] = a.state_grad ? a.state_grad[(size_t)r * ns + s] : 0.f;
#pragma unroll
   for (int k = 0; k < FZ_NPARAM; ++k) pb[k] = a.param_grad ? a.param_grad[(size_t)k * ns + s] : 0.f;
#pragma unroll
   for (int k = 0; k < FZ_NCONST; ++k) cb[k] = a.const_grad ? a.const_grad[(size_t)k * ns + s] : 0.f;
#if FZ_LOSS
   float ls = a.loss ? a.loss[s] : 0.f;                  // the stream's loss accumulator, in a register for the whole block
   const float gk = a.grad_scale;
#endif
   for (unsigned k = nck; k-- > 0;) {
      const size_t t0 = (size_t)k * FZ_C;
      const unsigned n = T - (unsigned)t0 < (unsigned)FZ_C ? T - (unsigned)t0 : (unsigned)FZ_C;   // rows of this chunk (1 .. FZ_C)
      float S[FZ_C][FZ_A(FZ_NSTATE)], X[FZ_C][FZ_A(FZ_NIN)];
      const float* ck = a.ckpt + (size_t)k * FZ_NSTATE * ns + s;
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
            for (int w = 0; w < FZ_NIN; ++w) X[j][w] = a.in[((t0 + j) * ns + s) * FZ_NIN + w];
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
            const size_t t = t0 + j;
            float yb[FZ_A(FZ_NOUT)], xb[FZ_A(FZ_NIN)];
            yb[0] = 0.f;
#if FZ_LOSS
            float y[FZ_A(FZ_NOUT)];
            y[0] = 0.f;
            fz_adj::out(X[j], c, p, S[j], y);
#pragma unroll
            for (int w = 0; w < FZ_NOUT; ++w) {            // the rule: slots in ascending order, one rounding per operation
               const float e = y[w] - a.target[(t * ns + s) * FZ_NOUT + w];
               yb[w] = e * gk;
               ls = ls + e * e;
            }
#else
#pragma unroll
            for (int w = 0; w < FZ_NOUT; ++w) yb[w] = a.out_grad[(t * ns + s) * FZ_NOUT + w];
#endif
            fz_adj::bwd(X[j], c, p, S[j], yb, xb, R, pb, cb);
            if (a.in_grad) {
#pragma unroll
               for (int w = 0; w < FZ_NIN; ++w) a.in_grad[(t * ns + s) * FZ_NIN + w] = xb[w];
            }
#if FZ_LOSS
            if (a.out) {                                    // (behind bwd(), like dL/dx: a store in front of it cost 60 and more registers)
#pragma unroll
               for (int w = 0; w < FZ_NOUT; ++w) a.out[(t * ns + s) * FZ_NOUT + w] = y[w];
            }
#endif
         }
   }
   if (a.state0_grad) {
#pragma unroll
      for (int r = 0; r < FZ_NSTATE; ++r) a.state0_grad[(size_t)r * ns + s] = R[r];
   }
   if (a.param_grad) {
#pragma unroll
      for (int k = 0; k < FZ_NPARAM; ++k) a.param_grad[(size_t)k * ns + s] = pb[k];
   }
   if (a.const_grad) {
#pragma unroll
      for (int k = 0; k < FZ_NCONST; ++k) a.const_grad[(size_t)k * ns + s] = cb[k];
   }
#if FZ_LOSS
   if (a.loss) a.loss[s] = ls;
#endif
}
