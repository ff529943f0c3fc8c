// fz_adjoint_ring_kernel / fz_adjoint_ring_loss_kernel -- hand-written gfx950 (MI355X, CDNA4) skeleton of the ADJOINT of one block whose
// graph has delay lines deeper than 8 samples (include/flowz_hip.h: fz_run_block_ring_grad), and with FZ_LOSS the same UNDER A
// SQUARED-ERROR LOSS (fz_run_block_ring_loss_grad): dL/dy formed in the kernel instead of read.  A sibling of fz_kernel_adjoint.hip.inc:
// the same two sweeps, the same order of every sum; what differs is where a deep line ("ring line": float, depth D in 9 .. 256) lives.
//
// One lane owns one stream for the whole block (wave64; the workgroups of the last wave are masked by the stream count).  A lane touches
// only its own LDS column, so there are no barriers and no atomics.
// The generated body (fz_codegen.cpp: gen_adjoint_body in ring mode) gives struct fz_adj with
//   fwd(x, c, p, s, rv, sn, u)                     the REGISTER state rows after one step and the ring lines' source values u[line],
//                                                  from the register rows before it, the step's frame and its ring-read values rv[read];
//   bwd(x, c, p, s, rv, yb, xb, R, pb, cb, ring, pt)   that step re-evaluated, then its adjoint statements in reverse node order;
//                                                  ring = the lane's LDS column, pt[line] = the row number modulo the line's depth;
//   out(x, c, p, s, rv, y)                         FZ_LOSS only: the step's output values (a delayed read of a ring line is rv[...], not
//                                                  a state row).
// Lines of depth <= 8 are what they are in fz_kernel_adjoint.hip.inc: state rows in registers (here COMPACT: register row r is the
// caller's state row fz_reg_row[r]), a checkpoint every FZ_C rows, the chunk re-run and walked backwards.
//
// A ring line l with source node u (state row row0 + j before row t is u[t-1-j], so a read at delay d of row t is u[t-d]):
//   its VALUES   sweep 1 keeps a value ring in LDS, as the forward kernels do (slot q mod D holds u[q]), and writes u[t] of every row
//                into the TAPE in the workspace, [T][n_ring_lines][n_streams], one coalesced row each.  Sweep 2 reads every ring value of
//                a chunk from the tape (row t - d; for t < d the caller's state row row0 + d - t - 1) together with the chunk's x rows:
//                the tape is the checkpoint of the ring rows.
//   its ADJOINTS sweep 2 keeps them in the SAME LDS ring (sweep 1 is done with it): slot q mod D holds the adjoint pending for u[q],
//                q running over negative positions too.  Before row T-1 the slot of u[T-1-j] holds state_grad[row0 + j] (+0.0f without
//                one); walking row t, rule 2 reads slot t and resets it to -0.0f, rule 3 adds each delayed read's adjoint into slot
//                t - d (a read at d = D finds the slot just reset); after row 0 the slot of u[-1-j] is state0_grad[row0 + j].
// LDS: ring[slot][lane], FZ_RING_SLOTS (the sum of the depths) x FZ_BLOCK floats; the lanes' dwords lie side by side and the slot is
// uniform over the wave: ds_read_b32 / ds_write_b32 without bank conflicts.
//
// FZ_LOSS: walking row t, sweep 2 holds the row's frame X[j], the register state rows S[j] and the ring-read values RV[j], so the row's
// outputs y are a few VALU instructions away.  Where the plain kernel reads a dL/dy row, the loss kernel reads the TARGET row and applies
// the rule of the header, per output slot w in ascending order:  e = y[w] - target[t][w];  ybar[w] = e * grad_scale;  loss = loss + e * e
// (each operation rounded once, no FMA).  ybar then enters bwd() as the dL/dy row does, so every gradient bit is fz_run_block_ring_grad's
// for that ybar.  The loss accumulator is one register per lane for the whole block, next to pb / cb: it starts from the caller's
// loss[stream] and runs over the rows T-1 .. 0 as they do, so blocks chain bitwise.  y leaves for `out` on the way if asked (the bits
// of fz_run_block).  The loss adds no LDS.
//
// Workspace: [ceil(T / FZ_C)][FZ_NREG][n_streams] checkpoints, then the tape [T][FZ_NRL][n_streams] (fz_program_ring_grad_workspace).
// HBM bytes per stream-sample: 4 (2 n_in + n_out + n_in) + 8 FZ_NREG / FZ_C + 4 FZ_NRL (the tape written) + 4 FZ_NRR (read back; the
// target read where dL/dy was), + 4 n_out when `out` is asked for.
//
// Compiled by hiprtc with the build options of the forward kernels: -ffp-contract=off (no FMA: one rounding per operation),
// correctly rounded division and square root, denormals kept.
#include "fz_graph_config.h"   // generated: FZ_NIN FZ_NOUT FZ_NCONST FZ_NPARAM FZ_NSTATE FZ_NREG FZ_NRL FZ_NRR FZ_RING_SLOTS FZ_C FZ_LOSS FZ_BLOCK
                               // FZ_KERNEL and the tables fz_reg_row, fz_rl_row0 / fz_rl_depth / fz_rl_slot0, fz_rr_line / fz_rr_delay

#define FZ_P 1
typedef float V;
typedef double VD;
#define FZ_A(n) ((n) > 0 ? (n) : 1)

#include "fz_graph_body.h"     // generated: struct fz_adj { fwd, bwd; FZ_LOSS: out }

struct fz_adj_ring_args {      // the layout of fz_adj_args (fz_kernel_adjoint.hip.inc): one host-side image serves both
   const float* in;            // [T][n_streams][n_in]
   const float* state;         // [n_state][n_streams]   the state before the block (register and ring lines' rows)
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
   float* ckpt;                // [n_chunks][FZ_NREG][n_streams] checkpoints, then [T][FZ_NRL][n_streams] the tape
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

extern "C" __global__ __launch_bounds__(FZ_BLOCK) void FZ_KERNEL(fz_adj_ring_args a)
{
   __shared__ float fz_ring[FZ_RING_SLOTS * FZ_BLOCK];
   const size_t ns = a.n_streams;
   const size_t s = (size_t)blockIdx.x * FZ_BLOCK + threadIdx.x;
   if (s >= ns) return;                                  // the masked tail of the last wave (no barriers below)
   float* const ring = fz_ring + threadIdx.x;            // the lane's column: slot q of line l is ring[(fz_rl_slot0[l] + q) * FZ_BLOCK]
   const unsigned T = a.n_samples, nck = a.n_chunks;
   float* const tape = a.ckpt + (size_t)nck * FZ_NREG * ns + s;
   float c[FZ_A(FZ_NCONST)], p[FZ_A(FZ_NPARAM)];
#pragma unroll
   for (int k = 0; k < FZ_NCONST; ++k) c[k] = a.c[k];
#pragma unroll
   for (int k = 0; k < FZ_NPARAM; ++k) p[k] = a.params[(size_t)k * ns + s];
   if (FZ_NCONST == 0) c[0] = 0.f;
   if (FZ_NPARAM == 0) p[0] = 0.f;

   // ---- sweep 1: forward over the block; the register rows before every chunk and every row's ring-line values into the workspace
   {
      float st[FZ_A(FZ_NREG)];
      unsigned pos[FZ_NRL];                                // the row number modulo each ring line's depth (uniform over the wave)
      st[0] = 0.f;
#pragma unroll
      for (int r = 0; r < FZ_NREG; ++r) st[r] = a.state[(size_t)fz_reg_row[r] * ns + s];
#pragma unroll
      for (int l = 0; l < FZ_NRL; ++l) {                   // the value rings: slot D - 1 - j holds u[-1-j], the caller's state row row0 + j
         const unsigned D = fz_rl_depth[l];
#pragma unroll 4
         for (unsigned j = 0; j < D; ++j) ring[(size_t)(fz_rl_slot0[l] + D - 1u - j) * FZ_BLOCK] = a.state[(size_t)(fz_rl_row0[l] + j) * ns + s];
         pos[l] = 0u;
      }
      for (unsigned k = 0; k < nck; ++k) {
         float* ck = a.ckpt + (size_t)k * FZ_NREG * ns + s;
#pragma unroll
         for (int r = 0; r < FZ_NREG; ++r) ck[(size_t)r * ns] = st[r];
         const size_t t0 = (size_t)k * FZ_C;
         const unsigned n = T - (unsigned)t0 < (unsigned)FZ_C ? T - (unsigned)t0 : (unsigned)FZ_C;   // rows of this chunk (1 .. FZ_C)
         float X[FZ_C][FZ_A(FZ_NIN)];
#pragma unroll
         for (int j = 0; j < FZ_C; ++j) {
            X[j][0] = 0.f;
            if ((unsigned)j < n) {
#pragma unroll
               for (int w = 0; w < FZ_NIN; ++w) X[j][w] = a.in[((t0 + j) * ns + s) * FZ_NIN + w];
            }
         }
#pragma unroll
         for (int j = 0; j < FZ_C; ++j)
            if ((unsigned)j < n) {
               float rv[FZ_A(FZ_NRR)], sn[FZ_A(FZ_NREG)], u[FZ_NRL];
               rv[0] = 0.f;
               sn[0] = 0.f;
#pragma unroll
               for (int q = 0; q < FZ_NRR; ++q) {
                  const unsigned l = fz_rr_line[q], d = fz_rr_delay[q], D = fz_rl_depth[l];
                  const unsigned slot = pos[l] >= d ? pos[l] - d : pos[l] + D - d;
                  rv[q] = ring[(size_t)(fz_rl_slot0[l] + slot) * FZ_BLOCK];
               }
               fz_adj::fwd(X[j], c, p, st, rv, sn, u);
#pragma unroll
               for (int l = 0; l < FZ_NRL; ++l) {
                  ring[(size_t)(fz_rl_slot0[l] + pos[l]) * FZ_BLOCK] = u[l];
                  tape[((t0 + j) * FZ_NRL + l) * ns] = u[l];
                  pos[l] = pos[l] + 1u == fz_rl_depth[l] ? 0u : pos[l] + 1u;
               }
#pragma unroll
               for (int r = 0; r < FZ_NREG; ++r) st[r] = sn[r];
            }
      }
   }

   // ---- sweep 2: chunks from the last to the first
   float R[FZ_A(FZ_NREG)], pb[FZ_A(FZ_NPARAM)], cb[FZ_A(FZ_NCONST)];
   R[0] = pb[0] = cb[0] = 0.f;
#pragma unroll
   for (int r = 0; r < FZ_NREG; ++r) R[r] = a.state_grad ? a.state_grad[(size_t)fz_reg_row[r] * ns + s] : 0.f;
#pragma unroll
   for (int k = 0; k < FZ_NPARAM; ++k) pb[k] = a.param_grad ? a.param_grad[(size_t)k * ns + s] : 0.f;
#pragma unroll
   for (int k = 0; k < FZ_NCONST; ++k) cb[k] = a.const_grad ? a.const_grad[(size_t)k * ns + s] : 0.f;
#if FZ_LOSS
   float ls = a.loss ? a.loss[s] : 0.f;                  // the stream's loss accumulator, in a register for the whole block
   const float gk = a.grad_scale;
#endif
#pragma unroll
   for (int l = 0; l < FZ_NRL; ++l) {                      // the adjoint rings: the slot of u[T-1-j] holds state_grad[row0 + j], or +0.0f
      const unsigned D = fz_rl_depth[l], top = (T - 1u) % D;
#pragma unroll 4
      for (unsigned j = 0; j < D; ++j) {
         const unsigned slot = top >= j ? top - j : top + D - j;
         ring[(size_t)(fz_rl_slot0[l] + slot) * FZ_BLOCK] = a.state_grad ? a.state_grad[(size_t)(fz_rl_row0[l] + j) * ns + s] : 0.f;
      }
   }
   for (unsigned k = nck; k-- > 0;) {
      const size_t t0 = (size_t)k * FZ_C;
      const unsigned n = T - (unsigned)t0 < (unsigned)FZ_C ? T - (unsigned)t0 : (unsigned)FZ_C;   // rows of this chunk (1 .. FZ_C)
      float S[FZ_C][FZ_A(FZ_NREG)], X[FZ_C][FZ_A(FZ_NIN)], RV[FZ_C][FZ_A(FZ_NRR)];
      const float* ck = a.ckpt + (size_t)k * FZ_NREG * ns + s;
#pragma unroll
      for (int j = 0; j < FZ_C; ++j) {
         S[j][0] = 0.f;
         X[j][0] = 0.f;
         RV[j][0] = 0.f;
      }
#pragma unroll
      for (int r = 0; r < FZ_NREG; ++r) S[0][r] = ck[(size_t)r * ns];
      // the chunk's frames and every ring read of the chunk, requested together: tape row t - d, or the caller's state for t < d
#pragma unroll
      for (int j = 0; j < FZ_C; ++j)
         if ((unsigned)j < n) {
#pragma unroll
            for (int w = 0; w < FZ_NIN; ++w) X[j][w] = a.in[((t0 + j) * ns + s) * FZ_NIN + w];
#pragma unroll
            for (int q = 0; q < FZ_NRR; ++q) {
               const unsigned l = fz_rr_line[q], d = fz_rr_delay[q];
               const size_t t = t0 + j;
               RV[j][q] = t >= d ? tape[((t - d) * FZ_NRL + l) * ns] : a.state[(size_t)(fz_rl_row0[l] + d - 1u - (unsigned)t) * ns + s];
            }
         }
#pragma unroll
      for (int j = 0; j + 1 < FZ_C; ++j)
         if ((unsigned)j + 1u < n) {
            float u[FZ_NRL];
            fz_adj::fwd(X[j], c, p, S[j], RV[j], S[j + 1], u);
         }
      // the saved states, frames and ring values are opaque from here on: the compiler must not keep the re-run's node values alive
      // for the backward walk instead of re-evaluating them from these
#pragma unroll
      for (int j = 0; j < FZ_C; ++j) {
#pragma unroll
         for (int r = 0; r < FZ_A(FZ_NREG); ++r) asm volatile("" : "+v"(S[j][r]));
#pragma unroll
         for (int w = 0; w < FZ_A(FZ_NIN); ++w) asm volatile("" : "+v"(X[j][w]));
#pragma unroll
         for (int q = 0; q < FZ_A(FZ_NRR); ++q) asm volatile("" : "+v"(RV[j][q]));
      }
      unsigned base[FZ_NRL];
#pragma unroll
      for (int l = 0; l < FZ_NRL; ++l) base[l] = (unsigned)t0 % fz_rl_depth[l];
#pragma unroll
      for (int j = FZ_C - 1; j >= 0; --j)
         if ((unsigned)j < n) {
            const size_t t = t0 + j;
            float yb[FZ_A(FZ_NOUT)], xb[FZ_A(FZ_NIN)];
            unsigned pt[FZ_NRL];
            yb[0] = 0.f;
#pragma unroll
            for (int l = 0; l < FZ_NRL; ++l) pt[l] = (base[l] + (unsigned)j) % fz_rl_depth[l];
#if FZ_LOSS
            float y[FZ_A(FZ_NOUT)];
            y[0] = 0.f;
            fz_adj::out(X[j], c, p, S[j], RV[j], y);
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
            fz_adj::bwd(X[j], c, p, S[j], RV[j], yb, xb, R, pb, cb, ring, pt);
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
      for (int r = 0; r < FZ_NREG; ++r) a.state0_grad[(size_t)fz_reg_row[r] * ns + s] = R[r];
#pragma unroll
      for (int l = 0; l < FZ_NRL; ++l) {                   // after row 0 the slot of u[-1-j] is D - 1 - j
         const unsigned D = fz_rl_depth[l];
#pragma unroll 4
         for (unsigned j = 0; j < D; ++j) a.state0_grad[(size_t)(fz_rl_row0[l] + j) * ns + s] = ring[(size_t)(fz_rl_slot0[l] + D - 1u - j) * FZ_BLOCK];
      }
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
