// fz_states_kernel, fz_states_ring_kernel, fz_states_far_kernel -- hand-written gfx950 (MI355X, CDNA4) skeleton of the BLOCK-START STATES
// of a recording: the first level of the two-level checkpointing of fz_run_recording_grad, fz_run_recording_ring_grad and
// fz_run_recording_far_grad / fz_run_recording_far_loss_grad (include/flowz_hip.h).  It runs the
// T rows forward like sweep 1 of fz_kernel_adjoint.hip.inc -- one lane owns one stream, the generated fz_adj::fwd (fz_codegen.cpp:
// gen_adjoint_body) is the step, so the state bits are the forward kernels' and sweep 1's -- and stores the state before rows 0, B, 2B,
// ... into starts[ceil(T / B)][n_state][n_streams], one coalesced row per state float, and the state after row T-1 into state_out if
// that is given.  It writes nothing else (FZ_FAR: but its working ring): no output frames, no checkpoints, no tape.
//
// Time-major frames [t][stream][wire]; state, parameter and coefficient rows [row][stream].  The workgroups of the last wave are masked
// by the stream count; no barriers.
//
// The recursion is one serial dependency chain per lane: a row's load cannot hide behind the row before it.  So the rows go in
// groups of FZ_U, and the x rows of the NEXT group are requested before the recursion of the current group runs (two groups of
// FZ_U * n_in registers); occupancy hides what is left.  Rows behind the last are fetched from row T-1 and not used (no branch around
// a load).  Whether a row starts a block is a comparison of two scalars (the row, the next block's first row).
//
// One text, three kernels: FZ_RING and, next to it, FZ_FAR (fz_graph_config.h) are the switches; a far kernel has both.  What the ring
// changes stands under `#if FZ_RING` below, five things: the LDS (its declaration, the lane's column, pos[]), the load of the state
// rows, what a block start stores, the step, what state_out stores.  What the far lines add to each of the five stands under
// `#if FZ_FAR`; without them FZ_NFL and FZ_NFR are 0 here.
//   FZ_RING 0: every delay line is at most 8 samples deep.  All n_state rows are register rows in the caller's order (FZ_NREG is
//     FZ_NSTATE, register row r the caller's row r), the step is fwd(x, c, p, st, sn), a start is one coalesced store per row.  No LDS.
//   FZ_RING 1: the graph has delay lines deeper than 8 samples, and the step is sweep 1 of fz_kernel_adjoint_ring.hip.inc, fz_adj::fwd
//     in ring mode.  Lines of depth <= 8 are register rows, COMPACT as in the ring adjoint kernel (register row r is the caller's state
//     row fz_reg_row[r]).  A ring line l with source node u keeps a value ring in the lane's LDS column: slot q mod D holds u[q], filled
//     from the caller's `state` (slot D - 1 - j holds u[-1-j], the state row row0 + j); pos[l], a scalar, is the row number modulo D.
//     Per row: the ring reads, then fz_adj::fwd, then one ds_write_b32 per line.  A lane touches only its own column: no barriers, no
//     atomics.  Where a row starts a block the register rows go to their caller rows and every ring line is read out of LDS in the
//     caller's order (fz_dump_state), row0 + j = ring[(pos - 1 - j) mod D], one coalesced store per row: D LDS reads and D stores per
//     line and block, D / B per row -- the price of a start.
//     LDS: ring[slot][lane], FZ_RING_SLOTS x FZ_BLOCK floats -- the ring adjoint kernel's bytes, so the same workgroups per CU.
//   FZ_FAR 1 (with FZ_RING 1): the graph has delay lines deeper than 256 samples as well, and the step is fz_adj::fwd in far mode:
//     rv[FZ_NRR + q] the value of far read q, u[FZ_NRL + f] the source value of far line f.  Register and ring lines are what they are
//     under FZ_RING, fz_dump_state included.  A FAR line f (float, source u, depth D, phase p0) fits neither registers nor LDS.  The
//     caller's D state rows of it are ring slots -- the value u[q] sits in slot (p0 + q) mod D, negative positions included -- and one
//     more row holds the phase.  The kernel keeps a WORKING VALUE RING of the line in the caller's workspace, in that same slot format:
//     row fz_fl_slot0[f] + k of the rows behind `starts` is slot k, one coalesced row per slot; the row offset is uniform over the
//     wave, the lane adds its stream.  Those rows are the head of the block workspace, which no launch has used yet when this kernel
//     runs (fz_grad.cpp: run_recording), and there are at least FZ_FAR_SLOTS of them whatever B is (fz_program_far_grad_workspace
//     counts the adjoint ring's rows among them).
//       filled   once, from `state`, by the identity map: slot k = state row row0 + k.
//       p0       the line's phase row of `state`, as the far adjoint kernel takes it: one readfirstlane per wave, reduced modulo D here,
//                so whatever the row holds no index leaves the line's rows.  fslot[f], a scalar, is the slot of the current row,
//                (p0 + t) mod D.
//       per row  one load per far read, slot (p0 + t - d) mod D, and one store per far line, u[t] into slot (p0 + t) mod D.
//       ahead    a read whose slot was written before the next group's rows are requested -- d >= 2 FZ_U, fz_fr_ahead[q]
//                (fz_codegen.cpp: far_read_with_next_group) -- is requested with them, two groups of FZ_U * FZ_NFR registers; a younger
//                read is a load of its own in front of its row.  Either way a lane reads only what it stored itself: same-lane program
//                order, as in sweep 1 of the far adjoint kernel.  Rows behind the last are requested from slots of the line (in bounds by
//                the modulus) and not used.
//       a start  the register rows and the LDS rings go out as under FZ_RING; the line's D slots are copied row for row to starts[k]
//                (the caller's slot format IS the working ring's) and the phase row is written as the forward writes it,
//                (float)((p0 + t) mod D) (fz_dump_far).  The same dump goes to state_out after row T-1.  D loads and D stores per line
//                and block: D / B per row.
//     The far lines use no LDS: fz_ring holds the ring lines' slots alone (none: no LDS at all).
//
// HBM bytes per stream-sample: 4 n_in + 4 n_state / B; FZ_FAR: + 4 FZ_NFL (the store of u) + 4 FZ_NFR (the far reads) + 4 FZ_FAR_SLOTS / B
// (the loads of a start's far slots), and once per recording 8 FZ_FAR_SLOTS / T for the fill.
//
// Compiled by hiprtc with the build options of every other kernel: -ffp-contract=off (no FMA: one rounding per operation), correctly
// rounded division and square root, denormals kept.
#include "fz_graph_config.h"   // generated: FZ_NIN FZ_NOUT FZ_NCONST FZ_NPARAM FZ_NSTATE FZ_RING FZ_U FZ_BLOCK FZ_KERNEL; with FZ_RING FZ_NREG FZ_NRL
                               // FZ_NRR FZ_RING_SLOTS FZ_FAR and the tables fz_reg_row, fz_rl_row0 / fz_rl_depth / fz_rl_slot0, fz_rr_line / fz_rr_delay;
                               // with FZ_FAR FZ_NFL FZ_NFR FZ_FAR_SLOTS and fz_fl_row0 / fz_fl_depth / fz_fl_slot0 / fz_fl_phase_row, fz_fr_line /
                               // fz_fr_delay / fz_fr_ahead

#define FZ_P 1
typedef float V;
typedef double VD;
#define FZ_A(n) ((n) > 0 ? (n) : 1)
#if FZ_RING
#define FZ_REG_ROW(r) fz_reg_row[r]           /* the caller's state row of register row r */
#if !FZ_FAR
#define FZ_NFL 0
#define FZ_NFR 0
#endif
#define FZ_NT (FZ_NRL + FZ_NFL)               /* source values a row hands out: the ring lines', then the far lines' */
#define FZ_NRV (FZ_NRR + FZ_NFR)              /* values a row reads: the ring reads, then the far reads */
#else
#define FZ_NREG FZ_NSTATE
#define FZ_REG_ROW(r) r
#endif

#include "fz_graph_body.h"     // generated: struct fz_adj { fwd, bwd }, in ring mode with FZ_RING, in far mode with FZ_FAR; fwd is all this kernel calls

struct fz_states_args {        // (one host-side image serves every mode)
   const float* in;            // [T][n_streams][n_in]
   const float* state;         // [n_state][n_streams]   the state before the recording (register rows, ring rows, far slots, phase rows)
   const float* params;        // [n_param][n_streams]
   float* starts;              // [ceil(T / B)][n_state][n_streams]   the state before rows 0, B, 2B, ...; FZ_FAR: behind it the working ring
   float* state_out;           // [n_state][n_streams]   the state after row T-1; null: not written
   unsigned long long n_streams;
   unsigned int n_samples;     // T >= 1
   unsigned int block_rows;    // B >= 1
   float c[FZ_A(FZ_NCONST)];   // the program's uniform coefficients
};

#if FZ_RING
//@splice fz_kernel_states_dump.hip.inc
#endif
#if FZ_FAR
//@splice fz_kernel_far.hip.inc
#endif

extern "C" __global__ __launch_bounds__(FZ_BLOCK) void FZ_KERNEL(fz_states_args a)
{
#if FZ_RING
#if FZ_RING_SLOTS > 0
   __shared__ float fz_ring[FZ_RING_SLOTS * FZ_BLOCK];
#endif
#endif
   const size_t ns = a.n_streams;
   const size_t s = (size_t)blockIdx.x * FZ_BLOCK + threadIdx.x;
   if (s >= ns) return;                                  // the masked tail of the last wave (no barriers below)
#if FZ_RING
#if FZ_RING_SLOTS > 0
   float* const ring = fz_ring + threadIdx.x;            // the lane's column: slot q of line l is ring[(fz_rl_slot0[l] + q) * FZ_BLOCK]
#else
   float* const ring = nullptr;                          // (far lines alone, no ring line: no LDS)
#endif
#endif
   const unsigned T = a.n_samples, B = a.block_rows;
#if FZ_FAR
   const unsigned nb = (T - 1u) / B + 1u;                // blocks: ceil(T / B)
   float* const wr = a.starts + (size_t)nb * FZ_NSTATE * ns + s;   // the lane's column of the working ring: slot k of far line f is wr[(fz_fl_slot0[f] + k) * ns]
   const float* const state = a.state + s;               // the lane's column of the caller's state, for the far lines' rows
#endif
   float c[FZ_A(FZ_NCONST)], p[FZ_A(FZ_NPARAM)], st[FZ_A(FZ_NREG)];
#pragma unroll
   for (int k = 0; k < FZ_NCONST; ++k) c[k] = a.c[k];
#pragma unroll
   for (int k = 0; k < FZ_NPARAM; ++k) p[k] = a.params[(size_t)k * ns + s];
   if (FZ_NCONST == 0) c[0] = 0.f;
   if (FZ_NPARAM == 0) p[0] = 0.f;
   st[0] = 0.f;
#pragma unroll
   for (int r = 0; r < FZ_NREG; ++r) st[r] = a.state[(size_t)FZ_REG_ROW(r) * ns + s];
#if FZ_RING
   unsigned pos[FZ_A(FZ_NRL)];                           // the row number modulo each ring line's depth (uniform over the wave)
   pos[0] = 0u;
#pragma unroll
   for (int l = 0; l < FZ_NRL; ++l) {                    // the value rings: slot D - 1 - j holds u[-1-j], the caller's state row row0 + j
      const unsigned D = fz_rl_depth[l];
#pragma unroll 4
      for (unsigned j = 0; j < D; ++j) ring[(size_t)(fz_rl_slot0[l] + D - 1u - j) * FZ_BLOCK] = a.state[(size_t)(fz_rl_row0[l] + j) * ns + s];
      pos[l] = 0u;
   }
#endif
#if FZ_FAR
   unsigned fslot[FZ_A(FZ_NFL)];                         // the slot of the current row of each far line, (p0 + t) mod D (uniform over the wave)
   fslot[0] = 0u;
#pragma unroll
   for (int f = 0; f < FZ_NFL; ++f) {                    // the working rings: the caller's slots as they are
      const unsigned D = fz_fl_depth[f];
      fslot[f] = __builtin_amdgcn_readfirstlane((unsigned)state[(size_t)fz_fl_phase_row[f] * ns]) % D;
#pragma unroll 4
      for (unsigned k = 0; k < D; ++k) wr[(size_t)(fz_fl_slot0[f] + k) * ns] = state[(size_t)(fz_fl_row0[f] + k) * ns];
   }
#endif

   float xa[FZ_U][FZ_A(FZ_NIN)], xb[FZ_U][FZ_A(FZ_NIN)];
#if FZ_FAR
   float fva[FZ_U][FZ_A(FZ_NFR)], fvb[FZ_U][FZ_A(FZ_NFR)];   // the far reads that travel with the x rows
#endif
#pragma unroll
   for (int j = 0; j < FZ_U; ++j) {
      xa[j][0] = xb[j][0] = 0.f;
#if FZ_FAR
      fva[j][0] = fvb[j][0] = 0.f;
#endif
      const size_t t = (unsigned)j < T ? (size_t)j : (size_t)T - 1;
#pragma unroll
      for (int w = 0; w < FZ_NIN; ++w) xa[j][w] = a.in[(t * ns + s) * FZ_NIN + w];
#if FZ_FAR
#pragma unroll
      for (int q = 0; q < FZ_NFR; ++q)
         if (fz_fr_ahead[q]) {
            const unsigned f = fz_fr_line[q], D = fz_fl_depth[f];
            fva[j][q] = wr[(size_t)(fz_fl_slot0[f] + fz_far_back(fz_far_on(fslot[f], (unsigned)j, D), fz_fr_delay[q], D)) * ns];
         }
#endif
   }
   unsigned tn = 0;                                      // the first row of the next block
   float* sk = a.starts + s;                             // its rows of `starts`
   for (unsigned t0 = 0; t0 < T; t0 += FZ_U) {
      // the next group's rows (FZ_FAR: and the far reads at least two groups old): requested here, used one trip on
#pragma unroll
      for (int j = 0; j < FZ_U; ++j) {
         const unsigned tj = t0 + FZ_U + j;
         const size_t t = tj < T ? (size_t)tj : (size_t)T - 1;
#pragma unroll
         for (int w = 0; w < FZ_NIN; ++w) xb[j][w] = a.in[(t * ns + s) * FZ_NIN + w];
#if FZ_FAR
#pragma unroll
         for (int q = 0; q < FZ_NFR; ++q)
            if (fz_fr_ahead[q]) {                        // (fslot is the slot of row t0 here; FZ_U + j < 2 FZ_U <= d <= D)
               const unsigned f = fz_fr_line[q], D = fz_fl_depth[f];
               fvb[j][q] = wr[(size_t)(fz_fl_slot0[f] + fz_far_back(fz_far_on(fslot[f], (unsigned)(FZ_U + j), D), fz_fr_delay[q], D)) * ns];
            }
#endif
      }
#pragma unroll
      for (int j = 0; j < FZ_U; ++j) {
         const unsigned t = t0 + j;
         if (t < T) {
            if (t == tn) {                               // (scalars both: no lane diverges)
#if FZ_RING
               fz_dump_state(sk, ns, st, ring, pos);
#if FZ_FAR
               fz_dump_far(sk, ns, wr, fslot);
#endif
#else
#pragma unroll
               for (int r = 0; r < FZ_NSTATE; ++r) sk[(size_t)r * ns] = st[r];
#endif
               sk += (size_t)FZ_NSTATE * ns;
               tn += B;
            }
#if FZ_RING
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
            for (int q = 0; q < FZ_NFR; ++q) {           // (a young read: the slot this lane stored a few rows ago)
               const unsigned f = fz_fr_line[q];
               rv[FZ_NRR + q] = fz_fr_ahead[q] ? fva[j][q] : wr[(size_t)(fz_fl_slot0[f] + fz_far_back(fslot[f], fz_fr_delay[q], fz_fl_depth[f])) * ns];
            }
#endif
            fz_adj::fwd(xa[j], c, p, st, rv, sn, u);
#pragma unroll
            for (int l = 0; l < FZ_NRL; ++l) {
               ring[(size_t)(fz_rl_slot0[l] + pos[l]) * FZ_BLOCK] = u[l];
               pos[l] = pos[l] + 1u == fz_rl_depth[l] ? 0u : pos[l] + 1u;
            }
#if FZ_FAR
#pragma unroll
            for (int f = 0; f < FZ_NFL; ++f) {
               wr[(size_t)(fz_fl_slot0[f] + fslot[f]) * ns] = u[FZ_NRL + f];
               fslot[f] = fslot[f] + 1u == fz_fl_depth[f] ? 0u : fslot[f] + 1u;
            }
#endif
#else
            float sn[FZ_A(FZ_NSTATE)];
            sn[0] = 0.f;
            fz_adj::fwd(xa[j], c, p, st, sn);
#endif
#pragma unroll
            for (int r = 0; r < FZ_NREG; ++r) st[r] = sn[r];
         }
      }
#pragma unroll
      for (int j = 0; j < FZ_U; ++j) {
#pragma unroll
         for (int w = 0; w < FZ_NIN; ++w) xa[j][w] = xb[j][w];
#if FZ_FAR
#pragma unroll
         for (int q = 0; q < FZ_NFR; ++q) fva[j][q] = fvb[j][q];
#endif
      }
   }
#if FZ_RING
   if (a.state_out) {
      fz_dump_state(a.state_out + s, ns, st, ring, pos);
#if FZ_FAR
      fz_dump_far(a.state_out + s, ns, wr, fslot);
#endif
   }
#else
   if (a.state_out) {
#pragma unroll
      for (int r = 0; r < FZ_NSTATE; ++r) a.state_out[(size_t)r * ns + s] = st[r];
   }
#endif
}
