// fz_states_sm_kernel, fz_states_ring_sm_kernel, fz_states_far_sm_kernel -- hand-written gfx950 (MI355X, CDNA4) skeleton of the BLOCK-START STATES of a
// recording on STREAM-MAJOR buffers (include/flowz_hip.h: fz_run_recording_grad with FZ_GRAD_STREAM_MAJOR,
// fz_run_recording_ring_grad_stream_major, fz_run_recording_far_grad_for with FZ_GRAD_STREAM_MAJOR).  What it computes and stores is fz_kernel_states.hip.inc's -- the T rows of the window
// forward with the generated fz_adj::fwd (fz_codegen.cpp: gen_adjoint_body), one lane per stream; the state before rows 0, B, 2B, ...
// of the window into starts[ceil(T / B)][n_state][n_streams] in the caller's row order, the state after the window's last row into
// state_out if that is given, nothing else (FZ_FAR: but its working ring) -- so the bits are the time-major kernel's.  What differs is how x arrives, and that is
// sweep 1 of fz_kernel_adjoint_sm.hip.inc:
//
// in is [n_streams][rows_total][n_in], the recording the window of rows [row0, row0 + n_samples).  The 64 lanes of a wave fetch a
// PATCH of [64 streams][FZ_R rows] as float4 pieces laid along the rows (consecutive lanes take consecutive pieces of one stream's
// run), park them in a wave-private LDS patch, and every lane reads its own row back in groups of FZ_U.  The patch carries x only: a
// patch row is FZ_R * n_in floats + 4 of padding, 64 (FZ_R n_in + 4) 4 bytes per wave.  FZ_R is a multiple of FZ_U (the rows of one
// unrolled group of the recursion) and of 4 (fz_grad.cpp: states_sm_patch_rows, ring_sm_geometry).  The fetch has no branches: a piece
// of a missing stream is fetched from the wave's last stream, a piece behind the window's last float from the head of its run, and
// both are parked where nobody reads them; at most FZ_AFLIGHT pieces are in flight per lane before they are parked.  There is no
// next-group prefetch of x into registers (xb of the time-major text): the patch is the prefetch.
//
// Masking, without a workgroup barrier (fz_wave_sync orders a wave's own LDS traffic; a wave past the last stream returns as a
// whole): the last wave's missing streams shadow the wave's last stream and store nothing; a last patch shorter than FZ_R runs
// the rows it has (a piece that straddles the window's last float is fetched whole: rows_total * n_in is a multiple of 4 floats, the
// piece ends inside the stream's buffer).  A block start (a comparison of two scalars: the row, the next block's first row) may fall
// anywhere in a patch and anywhere in an unrolled group.
//
// One text, three kernels: FZ_RING and, next to it, FZ_FAR (fz_graph_config.h) are the switches; a far kernel has both.  What the ring
// changes stands under `#if FZ_RING` below, five things: the LDS (its declaration, the lane's column, pos[]), the load of the state
// rows, what a block start stores, the step, what state_out stores.  What the far lines add to each stands under `#if FZ_FAR`;
// without them FZ_NFL and FZ_NFR are 0 here.
//   FZ_RING 0: every delay line is at most 8 samples deep.  All n_state rows are register rows in the caller's order (FZ_NREG is
//     FZ_NSTATE, register row r the caller's row r), the step is fwd(x, c, p, st, sn), a start is one coalesced store per row.  The LDS
//     is the waves' patches, fz_apatch[FZ_BLOCK / 64][64 * FZ_AROW]; a graph without input wires declares none.
//   FZ_RING 1: the graph has delay lines deeper than 8 samples; what the ring adds is the time-major text's with FZ_RING -- fz_adj::fwd
//     in ring mode, compact register rows (fz_reg_row), the value rings of the deep lines in the lane's LDS column, pos[], the ring
//     reads before and one ds_write_b32 per line after the step, fz_dump_state for a start and for state_out.  Where rings and patches
//     do not simply paste together (fz_kernel_adjoint_ring_sm.hip.inc has the same points):
//   * LDS is ONE static array: ring[slot][lane], FZ_RING_SLOTS x FZ_BLOCK floats, then the patches [FZ_BLOCK / 64][64 * FZ_AROW]
//     (FZ_BLOCK is whole waves: they start on a 256-byte boundary).  4 FZ_BLOCK (FZ_RING_SLOTS + FZ_R n_in + 4) bytes:
//     fz_grad.cpp: ring_sm_geometry chooses FZ_BLOCK and FZ_R together.  A graph without input wires declares no patch: the rings alone;
//   * idle lanes of the last wave shadow the wave's last stream (prow: its patch row, its state and params rows) but own the ring
//     column of their threadIdx.x; they store nothing -- no starts, no state_out -- and every address they form is in bounds.  A wave
//     past the last stream returns whole.  No workgroup barrier, no atomic: fz_wave_sync orders a wave's own patch traffic, a lane's
//     ring column is its own.
//   FZ_FAR 1 (with FZ_RING 1): the graph has delay lines deeper than 256 samples as well; what they add is the time-major text's with
//     FZ_FAR -- fz_adj::fwd in far mode (rv[FZ_NRR + q] the value of far read q, u[FZ_NRL + f] the source value of far line f), the
//     WORKING VALUE RING of every far line in the rows of the workspace behind `starts`, in the caller's slot format (row
//     fz_fl_slot0[f] + k is slot k, one coalesced [row][n_streams] row per slot; filled once from `state` by the identity map), fslot[],
//     the slot of the current row from one readfirstlane of the phase row reduced modulo D, per row one load per far read and one
//     store per far line, fz_dump_far behind fz_dump_state for a start and for state_out.  The far lines use no LDS: fz_ring holds the
//     ring lines' slots (none: the patches alone) and the patches.  Where this text differs from the time-major one:
//   * the patch is the prefetch for x, but the far reads still need one: a read whose slot was written before the next group's rows
//     are requested -- d >= 2 FZ_U, fz_fr_ahead[q] -- is requested for the NEXT group of FZ_U rows before the current group's
//     recursion runs (fva / fvb, two groups of FZ_U * FZ_NFR registers, carried across patch boundaries: FZ_R is a multiple of FZ_U,
//     so the groups tile the window whatever the patches do, and the slot depends on the row number alone).  A younger read is a load
//     of its own in front of its row.  Either way a lane reads only what it stored itself: same-lane program order.  Rows behind the
//     last are requested from slots of the line (in bounds by the modulus) and not used;
//   * idle lanes of the last wave shadow the wave's last stream for the working ring and the far rows of `state` as well (the
//     addresses are in bounds; what they read back is what that stream's lane stored or is about to store, and nothing depends on
//     it) and store nothing: no working-ring slots, the fill included, no starts, no state_out.
//
// HBM bytes per stream-sample: 4 n_in + 4 n_state / B, as the time-major text; FZ_FAR: + 4 FZ_NFL (the store of u) + 4 FZ_NFR (the far
// reads) + 4 FZ_FAR_SLOTS / B (the loads of a start's far slots), and once per recording 8 FZ_FAR_SLOTS / T for the fill.
//
// Compiled by hiprtc with the build options of every other kernel: -ffp-contract=off (no FMA: one rounding per operation), correctly
// rounded division and square root, denormals kept.
#include "fz_graph_config.h"   // generated: FZ_NIN FZ_NOUT FZ_NCONST FZ_NPARAM FZ_NSTATE FZ_RING FZ_U FZ_R FZ_BLOCK FZ_KERNEL; with FZ_RING FZ_NREG
                               // FZ_NRL FZ_NRR FZ_RING_SLOTS FZ_FAR and the tables fz_reg_row, fz_rl_row0 / fz_rl_depth / fz_rl_slot0, fz_rr_line /
                               // fz_rr_delay; with FZ_FAR FZ_NFL FZ_NFR FZ_FAR_SLOTS and fz_fl_row0 / fz_fl_depth / fz_fl_slot0 / fz_fl_phase_row,
                               // fz_fr_line / fz_fr_delay / fz_fr_ahead

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

#if (FZ_R % 4) != 0 || (FZ_R % FZ_U) != 0 || (FZ_BLOCK % 64) != 0
#error "stream-major states: the patch is a multiple of the unrolled group and of 4 rows, the workgroup whole waves"
#endif
#define FZ_AX (FZ_R * FZ_NIN)                 /* floats of x per patch row */
#define FZ_AROW (FZ_AX + 4)                   /* padded patch row */
#define FZ_API (FZ_AX / 4)                    /* float4 pieces per stream and patch */

//@splice fz_kernel_adjoint_patch.hip.inc   (the fetch is all this kernel uses of it)

struct fz_states_sm_args {     // (one host-side image serves every mode)
   const float* in;            // [n_streams][rows_total][n_in]
   const float* state;         // [n_state][n_streams]   the state before the recording (register rows, ring rows, far slots, phase rows)
   const float* params;        // [n_param][n_streams]
   float* starts;              // [ceil(T / B)][n_state][n_streams]   the state before rows 0, B, 2B, ... of the window; FZ_FAR: behind it the working ring
   float* state_out;           // [n_state][n_streams]   the state after the window's last row; null: not written
   unsigned long long n_streams;
   unsigned int n_samples;     // T >= 1
   unsigned int block_rows;    // B >= 1
   unsigned int rows_total;
   unsigned int row0;
   float c[FZ_A(FZ_NCONST)];   // the program's uniform coefficients
};

#if FZ_RING
//@splice fz_kernel_states_dump.hip.inc
#endif
#if FZ_FAR
//@splice fz_kernel_far.hip.inc
#endif

extern "C" __global__ __launch_bounds__(FZ_BLOCK) void FZ_KERNEL(fz_states_sm_args a)
{
#if FZ_RING
   // ring[slot][lane], then the waves' patches (FZ_RING_SLOTS * FZ_BLOCK floats are whole multiples of 256 bytes)
#if FZ_NIN > 0
   __shared__ __attribute__((aligned(16))) float fz_ring[FZ_RING_SLOTS * FZ_BLOCK + (FZ_BLOCK / 64) * 64 * FZ_AROW];
#elif FZ_RING_SLOTS > 0
   __shared__ float fz_ring[FZ_RING_SLOTS * FZ_BLOCK];
#endif
#else
#if FZ_NIN > 0
   __shared__ __attribute__((aligned(16))) float fz_apatch[FZ_BLOCK / 64][64 * FZ_AROW];
#endif
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
#if FZ_RING
#if FZ_RING_SLOTS > 0
   float* const ring = fz_ring + threadIdx.x;                 // the lane's OWN column (an idle lane's too): slot q of line l is ring[(fz_rl_slot0[l] + q) * FZ_BLOCK]
#else
   float* const ring = nullptr;                               // (far lines alone, no ring line: the LDS is the patches)
#endif
#endif
   const unsigned T = a.n_samples, B = a.block_rows;
#if FZ_FAR
   const unsigned nb = (T - 1u) / B + 1u;                     // blocks: ceil(T / B)
   float* const wr = a.starts + (size_t)nb * FZ_NSTATE * ns + s;   // the lane's column of the working ring (an idle lane: its shadow's): slot k of far line f is wr[(fz_fl_slot0[f] + k) * ns]
   const float* const state = a.state + s;                    // the lane's column of the caller's state, for the far lines' rows
#endif
   const unsigned npatch = (T + (unsigned)FZ_R - 1u) / (unsigned)FZ_R;
#if FZ_NIN > 0
#if FZ_RING
   float* const patch = fz_ring + FZ_RING_SLOTS * FZ_BLOCK + wave * (64u * FZ_AROW);
#else
   float* const patch = fz_apatch[wave];
#endif
   const float* const mine = patch + prow * FZ_AROW;
   const size_t istride = (size_t)a.rows_total * FZ_NIN;
   const float* const gin = a.in + s_base * istride + (size_t)a.row0 * FZ_NIN;   // the wave's first run: stream s_base, row row0
#endif

   float c[FZ_A(FZ_NCONST)], p[FZ_A(FZ_NPARAM)], st[FZ_A(FZ_NREG)];
#if FZ_RING
   unsigned pos[FZ_A(FZ_NRL)];                                // the row number modulo each ring line's depth (uniform over the wave)
#if FZ_FAR
   pos[0] = 0u;
#endif
#endif
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
#pragma unroll
   for (int l = 0; l < FZ_NRL; ++l) {                         // the value rings: slot D - 1 - j holds u[-1-j], the caller's state row row0 + j
      const unsigned D = fz_rl_depth[l];
#pragma unroll 4
      for (unsigned j = 0; j < D; ++j) ring[(size_t)(fz_rl_slot0[l] + D - 1u - j) * FZ_BLOCK] = a.state[(size_t)(fz_rl_row0[l] + j) * ns + s];
      pos[l] = 0u;
   }
#endif
#if FZ_FAR
   unsigned fslot[FZ_A(FZ_NFL)];                              // the slot of the current row of each far line, (p0 + t) mod D (uniform over the wave)
   fslot[0] = 0u;
#pragma unroll
   for (int f = 0; f < FZ_NFL; ++f) {                         // the working rings: the caller's slots as they are (an idle lane stores none)
      const unsigned D = fz_fl_depth[f];
      fslot[f] = __builtin_amdgcn_readfirstlane((unsigned)state[(size_t)fz_fl_phase_row[f] * ns]) % D;
      if (active) {
#pragma unroll 4
         for (unsigned k = 0; k < D; ++k) wr[(size_t)(fz_fl_slot0[f] + k) * ns] = state[(size_t)(fz_fl_row0[f] + k) * ns];
      }
   }
   float fva[FZ_U][FZ_A(FZ_NFR)], fvb[FZ_U][FZ_A(FZ_NFR)];    // the far reads that travel a group ahead: of the current group, of the next
#pragma unroll
   for (int j = 0; j < FZ_U; ++j) {
      fva[j][0] = fvb[j][0] = 0.f;
#pragma unroll
      for (int q = 0; q < FZ_NFR; ++q)
         if (fz_fr_ahead[q]) {
            const unsigned f = fz_fr_line[q], D = fz_fl_depth[f];
            fva[j][q] = wr[(size_t)(fz_fl_slot0[f] + fz_far_back(fz_far_on(fslot[f], (unsigned)j, D), fz_fr_delay[q], D)) * ns];
         }
   }
#endif

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
#if FZ_FAR
         // the far reads at least two groups old of the NEXT group's rows, in this patch or the next: requested here, used one trip on
#pragma unroll
         for (int j = 0; j < FZ_U; ++j) {
#pragma unroll
            for (int q = 0; q < FZ_NFR; ++q)
               if (fz_fr_ahead[q]) {                          // (fslot is the slot of row r0 + j0 here; FZ_U + j < 2 FZ_U <= d <= D)
                  const unsigned f = fz_fr_line[q], D = fz_fl_depth[f];
                  fvb[j][q] = wr[(size_t)(fz_fl_slot0[f] + fz_far_back(fz_far_on(fslot[f], (unsigned)(FZ_U + j), D), fz_fr_delay[q], D)) * ns];
               }
         }
#endif
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
#if FZ_RING
#if FZ_FAR
                  if (active) {
                     fz_dump_state(sk, ns, st, ring, pos);
                     fz_dump_far(sk, ns, wr, fslot);
                  }
#else
                  if (active) fz_dump_state(sk, ns, st, ring, pos);
#endif
#else
                  if (active) {
#pragma unroll
                     for (int r = 0; r < FZ_NSTATE; ++r) sk[(size_t)r * ns] = st[r];
                  }
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
               for (int q = 0; q < FZ_NFR; ++q) {             // (a young read: the slot this lane stored a few rows ago)
                  const unsigned f = fz_fr_line[q];
                  rv[FZ_NRR + q] = fz_fr_ahead[q] ? fva[j][q] : wr[(size_t)(fz_fl_slot0[f] + fz_far_back(fslot[f], fz_fr_delay[q], fz_fl_depth[f])) * ns];
               }
#endif
               fz_adj::fwd(x[j], c, p, st, rv, sn, u);
#pragma unroll
               for (int l = 0; l < FZ_NRL; ++l) {
                  ring[(size_t)(fz_rl_slot0[l] + pos[l]) * FZ_BLOCK] = u[l];
                  pos[l] = pos[l] + 1u == fz_rl_depth[l] ? 0u : pos[l] + 1u;
               }
#if FZ_FAR
#pragma unroll
               for (int f = 0; f < FZ_NFL; ++f) {
                  if (active) wr[(size_t)(fz_fl_slot0[f] + fslot[f]) * ns] = u[FZ_NRL + f];
                  fslot[f] = fslot[f] + 1u == fz_fl_depth[f] ? 0u : fslot[f] + 1u;
               }
#endif
#else
               float sn[FZ_A(FZ_NSTATE)];
               sn[0] = 0.f;
               fz_adj::fwd(x[j], c, p, st, sn);
#endif
#pragma unroll
               for (int r = 0; r < FZ_NREG; ++r) st[r] = sn[r];
            }
         }
#if FZ_FAR
#pragma unroll
         for (int j = 0; j < FZ_U; ++j) {
#pragma unroll
            for (int q = 0; q < FZ_NFR; ++q) fva[j][q] = fvb[j][q];
         }
#endif
      }
   }
#if FZ_RING
   if (a.state_out && active) fz_dump_state(a.state_out + s, ns, st, ring, pos);
#if FZ_FAR
   if (a.state_out && active) fz_dump_far(a.state_out + s, ns, wr, fslot);
#endif
#else
   if (a.state_out && active) {
#pragma unroll
      for (int r = 0; r < FZ_NSTATE; ++r) a.state_out[(size_t)r * ns + s] = st[r];
   }
#endif
}
