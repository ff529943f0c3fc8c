// fz_states_kernel -- hand-written gfx950 (MI355X, CDNA4) skeleton of the BLOCK-START STATES of a recording: the first level of the
// two-level checkpointing of fz_run_recording_grad (include/flowz_hip.h).  It runs the T rows forward like sweep 1 of
// fz_kernel_adjoint.hip.inc -- one lane owns one stream, the generated fz_adj::fwd (fz_codegen.cpp: gen_adjoint_body) is the step, so
// the state bits are the forward kernels' and sweep 1's -- and stores the state before rows 0, B, 2B, ... into
// starts[ceil(T / B)][n_state][n_streams], one coalesced row per state float, and the state after row T-1 into state_out if that is
// given.  It writes nothing else: no output frames, no checkpoints.
//
// Time-major frames [t][stream][wire]; state, parameter and coefficient rows [row][stream].  The workgroups of the last wave are masked
// by the stream count; no barriers.
//
// The recursion is one serial dependency chain per lane: a row's load cannot hide behind the row before it.  So the rows go in
// groups of FZ_U, and the x rows of the NEXT group are requested before the recursion of the current group runs (two groups of
// FZ_U * n_in registers); occupancy hides what is left.  Rows behind the last are fetched from row T-1 and not used (no branch around
// a load).  Whether a row starts a block is a comparison of two scalars (the row, the next block's first row).
//
// HBM bytes per stream-sample: 4 n_in + 4 n_state / B.
//
// Compiled by hiprtc with the build options of every other kernel: -ffp-contract=off (no FMA: one rounding per operation), correctly
// rounded division and square root, denormals kept.
#include "fz_graph_config.h"   // generated: FZ_NIN FZ_NOUT FZ_NCONST FZ_NPARAM FZ_NSTATE FZ_U FZ_BLOCK FZ_KERNEL

#define FZ_P 1
typedef float V;
typedef double VD;
#define FZ_A(n) ((n) > 0 ? (n) : 1)

#include "fz_graph_body.h"     // generated: struct fz_adj { fwd, bwd }; fwd is all this kernel calls

struct fz_states_args {
   const float* in;            // [T][n_streams][n_in]
   const float* state;         // [n_state][n_streams]   the state before the recording
   const float* params;        // [n_param][n_streams]
   float* starts;              // [ceil(T / B)][n_state][n_streams]   the state before rows 0, B, 2B, ...
   float* state_out;           // [n_state][n_streams]   the state after row T-1; null: not written
   unsigned long long n_streams;
   unsigned int n_samples;     // T >= 1
   unsigned int block_rows;    // B >= 1
   float c[FZ_A(FZ_NCONST)];   // the program's uniform coefficients
};

extern "C" __global__ __launch_bounds__(FZ_BLOCK) void FZ_KERNEL(fz_states_args a)
{
   const size_t ns = a.n_streams;
   const size_t s = (size_t)blockIdx.x * FZ_BLOCK + threadIdx.x;
   if (s >= ns) return;                                  // the masked tail of the last wave (no barriers below)
   const unsigned T = a.n_samples, B = a.block_rows;
   float c[FZ_A(FZ_NCONST)], p[FZ_A(FZ_NPARAM)], st[FZ_A(FZ_NSTATE)];
#pragma unroll
   for (int k = 0; k < FZ_NCONST; ++k) c[k] = a.c[k];
#pragma unroll
   for (int k = 0; k < FZ_NPARAM; ++k) p[k] = a.params[(size_t)k * ns + s];
   if (FZ_NCONST == 0) c[0] = 0.f;
   if (FZ_NPARAM == 0) p[0] = 0.f;
   st[0] = 0.f;
#pragma unroll
   for (int r = 0; r < FZ_NSTATE; ++r) st[r] = a.state[(size_t)r * ns + s];

   float xa[FZ_U][FZ_A(FZ_NIN)], xb[FZ_U][FZ_A(FZ_NIN)];
#pragma unroll
   for (int j = 0; j < FZ_U; ++j) {
      xa[j][0] = xb[j][0] = 0.f;
      const size_t t = (unsigned)j < T ? (size_t)j : (size_t)T - 1;
#pragma unroll
      for (int w = 0; w < FZ_NIN; ++w) xa[j][w] = a.in[(t * ns + s) * FZ_NIN + w];
   }
   unsigned tn = 0;                                      // the first row of the next block
   float* sk = a.starts + s;                             // its rows of `starts`
   for (unsigned t0 = 0; t0 < T; t0 += FZ_U) {
      // the next group's rows: requested here, used one trip on
#pragma unroll
      for (int j = 0; j < FZ_U; ++j) {
         const unsigned tj = t0 + FZ_U + j;
         const size_t t = tj < T ? (size_t)tj : (size_t)T - 1;
#pragma unroll
         for (int w = 0; w < FZ_NIN; ++w) xb[j][w] = a.in[(t * ns + s) * FZ_NIN + w];
      }
#pragma unroll
      for (int j = 0; j < FZ_U; ++j) {
         const unsigned t = t0 + j;
         if (t < T) {
            if (t == tn) {                               // (scalars both: no lane diverges)
#pragma unroll
               for (int r = 0; r < FZ_NSTATE; ++r) sk[(size_t)r * ns] = st[r];
               sk += (size_t)FZ_NSTATE * ns;
               tn += B;
            }
            float sn[FZ_A(FZ_NSTATE)];
            sn[0] = 0.f;
            fz_adj::fwd(xa[j], c, p, st, sn);
#pragma unroll
            for (int r = 0; r < FZ_NSTATE; ++r) st[r] = sn[r];
         }
      }
#pragma unroll
      for (int j = 0; j < FZ_U; ++j) {
#pragma unroll
         for (int w = 0; w < FZ_NIN; ++w) xa[j][w] = xb[j][w];
      }
   }
   if (a.state_out) {
#pragma unroll
      for (int r = 0; r < FZ_NSTATE; ++r) a.state_out[(size_t)r * ns + s] = st[r];
   }
}
