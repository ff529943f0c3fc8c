// fz_adjoint_ring_kernel / fz_adjoint_ring_loss_kernel and, with FZ_FAR, fz_adjoint_far_kernel / fz_adjoint_far_loss_kernel -- hand-written
// gfx950 (MI355X, CDNA4) skeleton of the ADJOINT of one block whose graph has delay lines deeper than 8 samples (include/flowz_hip.h:
// fz_run_block_ring_grad; FZ_FAR: deeper than 256 as well, fz_run_block_far_grad), and with FZ_LOSS the same UNDER A SQUARED-ERROR LOSS
// (fz_run_block_ring_loss_grad, fz_run_block_far_loss_grad): dL/dy formed in the kernel instead of read.  A sibling of
// fz_kernel_adjoint.hip.inc: the same two sweeps, the same order of every sum; what differs is where a deep line lives.
//
// One text, two switches (fz_graph_config.h): FZ_LOSS, and FZ_FAR -- 1 when the graph has FAR lines (float, depth D > 256), which fit
// neither registers nor LDS and keep their rings in HBM.  What the far lines add stands under `#if FZ_FAR`; without them FZ_NFL and
// FZ_NFR are 0 here and the text is the ring kernel alone.  Where a guard holds only a spelling (the place of a declaration, the ring
// lines' tape store), each mode keeps the statement order its kernels were compiled from: the machine code follows that order
// (tests/adjoint_code_pins.py).
//
// One lane owns one stream for the whole block (wave64; the workgroups of the last wave are masked by the stream count).  A lane touches
// only its own columns -- of LDS, of the workspace --, so there are no barriers and no atomics: plain loads and stores.
// The generated body (fz_codegen.cpp: gen_adjoint_body in ring / far mode) gives struct fz_adj with
//   fwd(x, c, p, s, rv, sn, u)                     the REGISTER state rows after one step and the deep lines' source values u[line],
//                                                  from the register rows before it, the step's frame and its delayed-read values rv[read];
//   bwd(x, c, p, s, rv, yb, xb, R, pb, cb, ring, pt)   that step re-evaluated, then its adjoint statements in reverse node order;
//                                                  ring = the lane's LDS column, pt[line] = the row number modulo the line's depth;
//   out(x, c, p, s, rv, y)                         FZ_LOSS only: the step's output values (a delayed read of a deep line is rv[...], not
//                                                  a state row).
//   FZ_FAR: rv[FZ_NRR + q] is the value of far read q (behind the ring reads), u[FZ_NRL + f] the source value of far line f (behind
//   the ring lines), and bwd() takes the far lines' pending adjoints behind pt:
//   bwd(..., ring, pt, fa, fpt, ns)   FZ_FAR_FAST 0: fa = the lane's column of the adjoint ring, fpt[f] = the slot of the row;
//   bwd(..., ring, pt, f2, fq)        FZ_FAR_FAST 1: f2[f] = rule 2's slot of the row, fq[q] = the pending adjoint read q adds into.
// Lines of depth <= 8 are what they are in fz_kernel_adjoint.hip.inc: state rows in registers (here COMPACT: register row r is the
// caller's state row fz_reg_row[r]), a checkpoint every FZ_C rows, the chunk re-run and walked backwards.
//
// A RING line l (float, depth D in 9 .. 256) with source node u (state row row0 + j before row t is u[t-1-j], so a read at delay d of
// row t is u[t-d]):
//   its VALUES   sweep 1 keeps a value ring in LDS, as the forward kernels do (slot q mod D holds u[q]), and writes u[t] of every row
//                into the TAPE in the workspace, [T][FZ_NT][n_streams], one coalesced row each.  Sweep 2 reads every ring value of
//                a chunk from the tape (row t - d; for t < d the caller's state row row0 + d - t - 1) together with the chunk's x rows:
//                the tape is the checkpoint of the ring rows.
//   its ADJOINTS sweep 2 keeps them in the SAME LDS ring (sweep 1 is done with it): slot q mod D holds the adjoint pending for u[q],
//                q running over negative positions too.  Before row T-1 the slot of u[T-1-j] holds state_grad[row0 + j] (+0.0f without
//                one); walking row t, rule 2 reads slot t and resets it to -0.0f, rule 3 adds each delayed read's adjoint into slot
//                t - d (a read at d = D finds the slot just reset); after row 0 the slot of u[-1-j] is state0_grad[row0 + j].
// LDS: ring[slot][lane], FZ_RING_SLOTS (the sum of the ring lines' depths) x FZ_BLOCK floats; the lanes' dwords lie side by side and the
// slot is uniform over the wave: ds_read_b32 / ds_write_b32 without bank conflicts.  The far lines use no LDS: a far graph without a
// ring line has none at all.
//
// A FAR line f with source u, depth D, phase p0: the caller's `depth` state rows are ring slots, the value u[q] sits in slot
// (p0 + q) mod D for every position q, negative ones included, before the block and after it.  p0 is the line's phase row of `state`,
// uniform over the streams (one readfirstlane per wave, as the forward takes it), reduced modulo D here: whatever the row holds, no
// index leaves the line's rows.
//   its VALUES   sweep 1 writes u[t] of every row into the TAPE, behind the ring lines' (tape line FZ_NRL + f).  A read at delay d of
//                row t is tape row t - d; for t < d the caller's state row row0 + (p0 + t - d) mod D (fz_far_value).  Sweep 1 keeps no
//                value ring: it reads the tape rows it wrote itself (the same lane, the same address: program order).  A read whose row
//                was written before the chunk began (fz_fr_chunked) is requested with the chunk's x rows, any other in front of its row.
//                Sweep 2 requests every far value of a chunk with the chunk's x rows, as it does the ring values.
//   its ADJOINTS live in the ADJOINT RING in the workspace, [FZ_FAR_SLOTS][n_streams] behind the tape: slot k of line f is row
//                fz_fl_slot0[f] + k, one coalesced row; the row offset is uniform over the wave, the lane adds its stream.  Before row
//                T-1 slot k holds state_grad[row0 + k] (+0.0f without one): the identity map, no permutation.  Walking row t, rule 2
//                reads slot (p0 + t) mod D and resets it to -0.0f, rule 3 adds each delayed read's adjoint into slot (p0 + t - d) mod D
//                (a read at d = D finds the slot just reset); after row 0 slot k goes to state0_grad[row0 + k], the phase row +0.0f.
//   FZ_FAR_FAST 1  no slot a chunk touches is touched twice within it (fz_codegen.cpp: far_fast_path): rule 2's slots and rule 3's
//                targets of the whole chunk are requested with its x and tape rows, the walk adds in registers, the stores leave once.
//   FZ_FAR_FAST 0  the per-row path: load, add, store in program order -- correct by the language's same-thread ordering, and a
//                dependent memory round trip per row.
//
// FZ_LOSS: walking row t, sweep 2 holds the row's frame X[j], the register state rows S[j] and the delayed-read values RV[j], so the
// row's outputs y are a few VALU instructions away.  Where the plain kernel reads a dL/dy row, the loss kernel reads the TARGET row and
// applies the rule of the header, per output slot w in ascending order:  e = y[w] - target[t][w];  ybar[w] = e * grad_scale;
// loss = loss + e * e  (each operation rounded once, no FMA).  ybar then enters bwd() as the dL/dy row does, so every gradient bit is
// fz_run_block_ring_grad's (fz_run_block_far_grad's) for that ybar.  The loss accumulator is one register per lane for the whole block,
// next to pb / cb: it starts from the caller's loss[stream] and runs over the rows T-1 .. 0 as they do, so blocks chain bitwise.  y
// leaves for `out` on the way if asked (the bits of fz_run_block).  The loss adds no LDS.
//
// Workspace: [ceil(T / FZ_C)][FZ_NREG][n_streams] checkpoints, then the tape [T][FZ_NRL + FZ_NFL][n_streams], then (FZ_FAR) the adjoint
// ring [FZ_FAR_SLOTS][n_streams] (fz_program_ring_grad_workspace, fz_program_far_grad_workspace).
// HBM bytes per stream-sample: 4 (2 n_in + n_out + n_in) + 8 FZ_NREG / FZ_C + 4 FZ_NRL (the tape written) + 4 FZ_NRR (read back; the
// target read where dL/dy was), + 4 n_out when `out` is asked for.  FZ_FAR: the far lines count among the ring lines and the far reads
// among the ring reads, + 4 FZ_NFR (sweep 1 reads its values from the tape too), + the adjoint ring's traffic: 4 FZ_NFL (rule 2's slot
// read) + 8 FZ_NFR (rule 3's targets read and written) - 4 per read at the full depth (not read: the slot just reset; on the fast path
// its store is the reset's as well); and once per block 8 FZ_FAR_SLOTS / T (the ring filled and emptied) + the 4 FZ_FAR_SLOTS / T of
// state_grad and state0_grad each.
//
// Compiled by hiprtc with the build options of the forward kernels: -ffp-contract=off (no FMA: one rounding per operation),
// correctly rounded division and square root, denormals kept.
#include "fz_graph_config.h"   // generated: FZ_NIN FZ_NOUT FZ_NCONST FZ_NPARAM FZ_NSTATE FZ_NREG FZ_NRL FZ_NRR FZ_RING_SLOTS FZ_FAR FZ_C FZ_LOSS FZ_BLOCK
                               // FZ_KERNEL and the tables fz_reg_row, fz_rl_row0 / fz_rl_depth / fz_rl_slot0, fz_rr_line / fz_rr_delay; with FZ_FAR
                               // FZ_NFL FZ_NFR FZ_FAR_SLOTS FZ_FAR_FAST and fz_fl_row0 / fz_fl_depth / fz_fl_slot0 / fz_fl_phase_row, fz_fr_line /
                               // fz_fr_delay / fz_fr_chunked

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

struct fz_adj_ring_args {      // the layout of fz_adj_args (fz_kernel_adjoint.hip.inc): one host-side image serves the family, both modes
   const float* in;            // [T][n_streams][n_in]
   const float* state;         // [n_state][n_streams]   the state before the block (register rows, ring rows, far slots, phase rows)
   const float* params;        // [n_param][n_streams]
#if FZ_LOSS
   const float* target;        // [T][n_streams][n_out]  what y is compared with
#else
   const float* out_grad;      // [T][n_streams][n_out]
#endif
   const float* state_grad;    // [n_state][n_streams]   dL/d(state after the block); null: zero.  A far line's phase row is never read
   float* in_grad;             // [T][n_streams][n_in]   written; null: not computed
   float* state0_grad;         // [n_state][n_streams]   written; null: not computed (may be state_grad)
   float* param_grad;          // [n_param][n_streams]   added to; null: not computed
   float* const_grad;          // [n_const][n_streams]   added to; null: not computed
   float* ckpt;                // the workspace: [n_chunks][FZ_NREG][n_streams] checkpoints, [T][FZ_NT][n_streams] the tape, FZ_FAR: the adjoint ring
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

#if FZ_FAR
//@splice fz_kernel_far.hip.inc
#endif

extern "C" __global__ __launch_bounds__(FZ_BLOCK) void FZ_KERNEL(fz_adj_ring_args a)
{
#if FZ_RING_SLOTS > 0
   __shared__ float fz_ring[FZ_RING_SLOTS * FZ_BLOCK];
#endif
   const size_t ns = a.n_streams;
   const size_t s = (size_t)blockIdx.x * FZ_BLOCK + threadIdx.x;
   if (s >= ns) return;                                  // the masked tail of the last wave (no barriers below)
#if FZ_RING_SLOTS > 0
   float* const ring = fz_ring + threadIdx.x;            // the lane's column: slot q of line l is ring[(fz_rl_slot0[l] + q) * FZ_BLOCK]
#else
   float* const ring = nullptr;                          // (no ring line: no LDS)
#endif
   const unsigned T = a.n_samples, nck = a.n_chunks;
   float* const tape = a.ckpt + (size_t)nck * FZ_NREG * ns + s;
#if FZ_FAR
   float* const fa = tape + (size_t)T * FZ_NT * ns;      // the lane's column of the adjoint ring: row k is fa[k * ns]
   const float* const state = a.state + s;               // the lane's column of the caller's state, for the far lines' rows
#endif
   float c[FZ_A(FZ_NCONST)], p[FZ_A(FZ_NPARAM)];
#pragma unroll
   for (int k = 0; k < FZ_NCONST; ++k) c[k] = a.c[k];
#pragma unroll
   for (int k = 0; k < FZ_NPARAM; ++k) p[k] = a.params[(size_t)k * ns + s];
   if (FZ_NCONST == 0) c[0] = 0.f;
   if (FZ_NPARAM == 0) p[0] = 0.f;
#if FZ_FAR
   unsigned fp0[FZ_A(FZ_NFL)];                           // the far lines' phases before the block, modulo their depths
   fp0[0] = 0u;
#pragma unroll
   for (int f = 0; f < FZ_NFL; ++f)
      fp0[f] = __builtin_amdgcn_readfirstlane((unsigned)state[(size_t)fz_fl_phase_row[f] * ns]) % fz_fl_depth[f];
#endif

   // ---- sweep 1: forward over the block; the register rows before every chunk and every row's ring- and far-line values into the workspace
   {
      float st[FZ_A(FZ_NREG)];
      unsigned pos[FZ_A(FZ_NRL)];                          // the row number modulo each ring line's depth (uniform over the wave)
      st[0] = 0.f;
      pos[0] = 0u;
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
         float X[FZ_C][FZ_A(FZ_NIN)], FV[FZ_C][FZ_A(FZ_NFR)];
         // the chunk's frames (FZ_FAR: and the far reads whose rows were written before the chunk began, requested together)
#pragma unroll
         for (int j = 0; j < FZ_C; ++j) {
            X[j][0] = 0.f;
            FV[j][0] = 0.f;
            if ((unsigned)j < n) {
#pragma unroll
               for (int w = 0; w < FZ_NIN; ++w) X[j][w] = a.in[((t0 + j) * ns + s) * FZ_NIN + w];
#if FZ_FAR
#pragma unroll
               for (int q = 0; q < FZ_NFR; ++q)
                  if (fz_fr_chunked[q]) FV[j][q] = fz_far_value(tape, state, ns, fp0, q, t0 + j);
#endif
            }
         }
#pragma unroll
         for (int j = 0; j < FZ_C; ++j)
            if ((unsigned)j < n) {
               float rv[FZ_A(FZ_NRV)], sn[FZ_A(FZ_NREG)], u[FZ_A(FZ_NT)];
               rv[0] = 0.f;
               sn[0] = 0.f;
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
               fz_adj::fwd(X[j], c, p, st, rv, sn, u);
#pragma unroll
               for (int l = 0; l < FZ_NRL; ++l) {
                  ring[(size_t)(fz_rl_slot0[l] + pos[l]) * FZ_BLOCK] = u[l];
#if !FZ_FAR
                  tape[((t0 + j) * FZ_NT + l) * ns] = u[l];
#endif
                  pos[l] = pos[l] + 1u == fz_rl_depth[l] ? 0u : pos[l] + 1u;
               }
#if FZ_FAR
#pragma unroll
               for (int l = 0; l < FZ_NT; ++l) tape[((t0 + j) * FZ_NT + l) * ns] = u[l];   // (the ring lines' values, then the far lines')
#endif
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
   for (int l = 0; l < FZ_NRL; ++l) {                      // the adjoint rings in LDS: the slot of u[T-1-j] holds state_grad[row0 + j], or +0.0f
      const unsigned D = fz_rl_depth[l], top = (T - 1u) % D;
#pragma unroll 4
      for (unsigned j = 0; j < D; ++j) {
         const unsigned slot = top >= j ? top - j : top + D - j;
         ring[(size_t)(fz_rl_slot0[l] + slot) * FZ_BLOCK] = a.state_grad ? a.state_grad[(size_t)(fz_rl_row0[l] + j) * ns + s] : 0.f;
      }
   }
#if FZ_FAR
#pragma unroll
   for (int f = 0; f < FZ_NFL; ++f) {                      // the adjoint ring in the workspace: slot k holds state_grad[row0 + k], or +0.0f
      const unsigned D = fz_fl_depth[f];
#pragma unroll 4
      for (unsigned k = 0; k < D; ++k)
         fa[(size_t)(fz_fl_slot0[f] + k) * ns] = a.state_grad ? a.state_grad[(size_t)(fz_fl_row0[f] + k) * ns + s] : 0.f;
   }
#endif
   for (unsigned k = nck; k-- > 0;) {
      const size_t t0 = (size_t)k * FZ_C;
      const unsigned n = T - (unsigned)t0 < (unsigned)FZ_C ? T - (unsigned)t0 : (unsigned)FZ_C;   // rows of this chunk (1 .. FZ_C)
      float S[FZ_C][FZ_A(FZ_NREG)], X[FZ_C][FZ_A(FZ_NIN)], RV[FZ_C][FZ_A(FZ_NRV)];
      const float* ck = a.ckpt + (size_t)k * FZ_NREG * ns + s;
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
      // the chunk's frames and every ring and far read of the chunk, requested together: tape row t - d, or the caller's state for
      // t < d; on the fast path the chunk's slots of the adjoint ring as well
#pragma unroll
      for (int j = 0; j < FZ_C; ++j)
         if ((unsigned)j < n) {
#if FZ_FAR
            const size_t t = t0 + j;                        // (far mode: in front of the x loads, ring mode: behind them -- the machine code follows the place, and each mode keeps its own)
#endif
#pragma unroll
            for (int w = 0; w < FZ_NIN; ++w) X[j][w] = a.in[((t0 + j) * ns + s) * FZ_NIN + w];
#if !FZ_FAR
            const size_t t = t0 + j;
#endif
#pragma unroll
            for (int q = 0; q < FZ_NRR; ++q) {
               const unsigned l = fz_rr_line[q], d = fz_rr_delay[q];
               RV[j][q] = t >= d ? tape[((t - d) * FZ_NT + l) * ns] : a.state[(size_t)(fz_rl_row0[l] + d - 1u - (unsigned)t) * ns + s];
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
            const size_t t = t0 + j;
            float yb[FZ_A(FZ_NOUT)], xb[FZ_A(FZ_NIN)];
            unsigned pt[FZ_A(FZ_NRL)], fpt[FZ_A(FZ_NFL)];   // per ring line: the row number modulo its depth; per far line: the slot of the row
            yb[0] = 0.f;
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
            for (int w = 0; w < FZ_NOUT; ++w) {            // the rule: slots in ascending order, one rounding per operation
               const float e = y[w] - a.target[(t * ns + s) * FZ_NOUT + w];
               yb[w] = e * gk;
               ls = ls + e * e;
            }
#else
#pragma unroll
            for (int w = 0; w < FZ_NOUT; ++w) yb[w] = a.out_grad[(t * ns + s) * FZ_NOUT + w];
#endif
#if !FZ_FAR
            fz_adj::bwd(X[j], c, p, S[j], RV[j], yb, xb, R, pb, cb, ring, pt);
#elif FZ_FAR_FAST
            fz_adj::bwd(X[j], c, p, S[j], RV[j], yb, xb, R, pb, cb, ring, pt, F2[j], FQ[j]);
            // the row's slots leave once: rule 2's reset, then what rule 3 made of its targets.  A read at the full depth targets the
            // slot its row just reset -- and a line's depth is its deepest read, so there is one unless the graph was lowered otherwise:
            // then the reset itself never leaves
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
#else
            fz_adj::bwd(X[j], c, p, S[j], RV[j], yb, xb, R, pb, cb, ring, pt, fa, fpt, ns);
#endif
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
#if FZ_FAR
#pragma unroll
      for (int f = 0; f < FZ_NFL; ++f) {                   // the far lines: slot k as it is, the phase row +0.0f
         const unsigned D = fz_fl_depth[f];
#pragma unroll 4
         for (unsigned k = 0; k < D; ++k) a.state0_grad[(size_t)(fz_fl_row0[f] + k) * ns + s] = fa[(size_t)(fz_fl_slot0[f] + k) * ns];
         a.state0_grad[(size_t)fz_fl_phase_row[f] * ns + s] = 0.f;
      }
#endif
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
