// fz_block_kernel -- hand-written gfx950 (MI355X, CDNA4) skeleton of the fused Flowz block kernel.
//
// One launch evaluates a whole flow-graph for FZ_U-sample chunks over n_samples samples of
// n_streams independent streams: the reference's per-sample call stateful_lambda::operator()
// (flowz/flowz.hpp:1225-1229) plus its caller's sample loop (test/benchmark.cpp:137-147).
//
// Mapping (MI355X-first, nothing here resembles the reference's tuple recursion):
//   * one wavefront lane owns FZ_P adjacent streams for the whole block; with FZ_P == 2 every
//     graph node is ONE packed instruction (v_pk_mul_f32 / v_pk_add_f32) for two streams; with
//     few streams (FZ_SKEW, one stream per lane) the packed halves are instead pairs of isomorphic
//     graph segments running one sample apart (stage packing, see the FZ_SKEW block below);
//   * delay lines up to 8 deep live in VGPRs (the generated step() renames them, the unrolled
//     chunk leaves no v_mov); deeper lines are LDS ring buffers, one column per lane (a lane
//     touches only its own column: no barriers, no bank conflicts); uniform coefficients sit in
//     the kernarg segment (SGPRs), per-stream coefficients in VGPRs;
//   * frames are time-major [t][stream][wire], optionally in stream tiles [tile][t][stream][wire]
//     (32 KiB row segments stream measurably faster from HBM than 4 MiB rows): a wave reads
//     64*FZ_P*n_in contiguous floats per time step with one buffer load per lane (ONE descriptor
//     per chunk in SGPRs, constant 32-bit lane offset, the row inside the chunk in the load's
//     scalar offset: no per-step address arithmetic); rows are software-prefetched one chunk (FZ_U
//     steps) ahead through two register buffers (A/B ping-pong, fully unrolled: no copies); loads
//     are non-temporal, stores nt|sc1; blocks map to XCDs in contiguous stream ranges;
//   * a second kernel body (FZ_VF_STREAM_MAJOR) takes stream-major buffers [stream][t][wire] and
//     transposes chunks through wave-private LDS patches;
//   * state [n_state][n_streams] is read once at block start and written once at the end, so
//     blocks chain and the host can snapshot it (the closure-copy of flowz.hpp:1206);
//   * arithmetic is compiled with -ffp-contract=off: one IEEE float32 rounding per graph node
//     in the user's association order (proto::_default, flowz.hpp:769-772); denormals kept.
//
// This text is compiled twice: by hiprtc at run time with the generated headers
// "fz_graph_config.h" / "fz_graph_body.h" of the graph at hand, and by hipcc in build() with a
// sample graph (the 6-stage DF1 cascade) as a compile check.
#include "fz_graph_config.h"   // generated: FZ_NIN FZ_NOUT FZ_NCONST FZ_NPARAM FZ_P FZ_U FZ_BLOCK FZ_FLAGS FZ_LDS_SLOTS FZ_SKEW FZ_MINWAVES FZ_KERNEL

#define FZ_VF_OUT_F64 64u
#define FZ_VF_PREFETCH3 32u
#define FZ_VF_STREAM_MAJOR 128u
#define FZ_VF_SM_LONG 256u
#define FZ_VF_WAVE_SPLIT 1024u
#define FZ_VF_WAVE_SPLIT3 2048u
#define FZ_VF_IO_WAVE 32768u
#define FZ_VF_LOCKSTEP 524288u
#define FZ_VF_GRID_SYNC 8388608u
#define FZ_VF_RAGGED 268435456u
#define FZ_VF_ST_MERGE 536870912u
#define FZ_VF_IO_WAVE2 33554432u
#define FZ_VF_LANE_PAIRS 1073741824u
#define FZ_VF_LANE_SINGLES 2147483648u
// LANE GROUPS: the lane's FZ_P streams are FZ_P / FZ_LG groups of FZ_LG adjacent streams, the groups 64 x FZ_LG streams apart (the wave still
// covers 64 x FZ_P adjacent streams: group k of lane l starts at the wave's first stream + (64 k + l) x FZ_LG).  Every frame / state access
// of a lane is then one access per group, each contiguous ACROSS the lanes of the wave -- whole sectors per instruction where the lane's
// own slice would be wider than 16 bytes.  FZ_VF_LANE_PAIRS: groups of two (four streams per lane, 8-byte frames); FZ_VF_LANE_SINGLES:
// groups of one (two or four streams per lane, 16-byte frames).  FZ_PAIRS = 1 says "grouped", whatever the group size.
#if FZ_FLAGS & FZ_VF_LANE_PAIRS
#define FZ_PAIRS 1
#define FZ_LG 2
#elif FZ_FLAGS & FZ_VF_LANE_SINGLES
#define FZ_PAIRS 1
#define FZ_LG 1
#else
#define FZ_PAIRS 0
#define FZ_LG FZ_P
#endif
#define FZ_NGRP (FZ_P / FZ_LG)

typedef float fz_f2 __attribute__((ext_vector_type(2)));
typedef float fz_f4 __attribute__((ext_vector_type(4)));
typedef unsigned fz_u2 __attribute__((ext_vector_type(2)));
typedef unsigned fz_u4 __attribute__((ext_vector_type(4)));

#if FZ_P == 1
typedef float V;
#elif FZ_P == 2
typedef fz_f2 V;
#elif FZ_P == 4
typedef fz_f4 V;
#else
#error "FZ_P must be 1, 2 or 4"
#endif
// float64 companions of V: nodes below a C++ `double` literal evaluate in double (one IEEE
// rounding per node as well, no v_fma_f64); delay lines and frames stay float32
typedef double fz_d2 __attribute__((ext_vector_type(2)));
typedef double fz_d4 __attribute__((ext_vector_type(4)));
#if FZ_P == 1
typedef double VD;
__device__ __forceinline__ VD fz_cvt_d(V v) { return (double)v; }
__device__ __forceinline__ V fz_cvt_f(VD v) { return (float)v; }
#elif FZ_P == 2
typedef fz_d2 VD;
__device__ __forceinline__ VD fz_cvt_d(V v) { return __builtin_convertvector(v, VD); }
__device__ __forceinline__ V fz_cvt_f(VD v) { return __builtin_convertvector(v, V); }
#else
typedef fz_d4 VD;
__device__ __forceinline__ VD fz_cvt_d(V v) { return __builtin_convertvector(v, VD); }
__device__ __forceinline__ V fz_cvt_f(VD v) { return __builtin_convertvector(v, V); }
#endif

// typed programs (fz_compile_typed): a double travels through frames and state as two 32-bit words
__device__ __forceinline__ double fz_join1(float lo, float hi)
{
   return __builtin_bit_cast(double, (unsigned long long)__builtin_bit_cast(unsigned, lo) | ((unsigned long long)__builtin_bit_cast(unsigned, hi) << 32));
}
__device__ __forceinline__ float fz_lo1(double v) { return __builtin_bit_cast(float, (unsigned)__builtin_bit_cast(unsigned long long, v)); }
__device__ __forceinline__ float fz_hi1(double v) { return __builtin_bit_cast(float, (unsigned)(__builtin_bit_cast(unsigned long long, v) >> 32)); }
#if FZ_P == 1
__device__ __forceinline__ VD fz_join_d(V lo, V hi) { return fz_join1(lo, hi); }
__device__ __forceinline__ V fz_lo_d(VD v) { return fz_lo1(v); }
__device__ __forceinline__ V fz_hi_d(VD v) { return fz_hi1(v); }
#else
__device__ __forceinline__ VD fz_join_d(V lo, V hi)
{
   VD r;
#pragma unroll
   for (int j = 0; j < FZ_P; ++j) r[j] = fz_join1(lo[j], hi[j]);
   return r;
}
__device__ __forceinline__ V fz_lo_d(VD v)
{
   V r;
#pragma unroll
   for (int j = 0; j < FZ_P; ++j) r[j] = fz_lo1(v[j]);
   return r;
}
__device__ __forceinline__ V fz_hi_d(VD v)
{
   V r;
#pragma unroll
   for (int j = 0; j < FZ_P; ++j) r[j] = fz_hi1(v[j]);
   return r;
}
#endif
// the data-dependent branch of __divdc3 (Smith's method): |a| < |b| as 1.0 / 0.0, and the selection by such a mask
#if FZ_P == 1
__device__ __forceinline__ VD fz_abs_lt(VD a, VD b) { return __builtin_fabs(a) < __builtin_fabs(b) ? 1.0 : 0.0; }
__device__ __forceinline__ VD fz_select(VD m, VD x, VD y) { return m != 0.0 ? x : y; }
__device__ __forceinline__ V fz_abs_lt(V a, V b) { return __builtin_fabsf(a) < __builtin_fabsf(b) ? 1.f : 0.f; }
__device__ __forceinline__ V fz_select(V m, V x, V y) { return m != 0.f ? x : y; }
#else
__device__ __forceinline__ VD fz_abs_lt(VD a, VD b)
{
   VD r;
#pragma unroll
   for (int j = 0; j < FZ_P; ++j) r[j] = __builtin_fabs(a[j]) < __builtin_fabs(b[j]) ? 1.0 : 0.0;
   return r;
}
__device__ __forceinline__ VD fz_select(VD m, VD x, VD y)
{
   VD r;
#pragma unroll
   for (int j = 0; j < FZ_P; ++j) r[j] = m[j] != 0.0 ? x[j] : y[j];
   return r;
}
__device__ __forceinline__ V fz_abs_lt(V a, V b)
{
   V r;
#pragma unroll
   for (int j = 0; j < FZ_P; ++j) r[j] = __builtin_fabsf(a[j]) < __builtin_fabsf(b[j]) ? 1.f : 0.f;
   return r;
}
__device__ __forceinline__ V fz_select(V m, V x, V y)
{
   V r;
#pragma unroll
   for (int j = 0; j < FZ_P; ++j) r[j] = m[j] != 0.f ? x[j] : y[j];
   return r;
}
#endif
// a state row of n_streams doubles (two float rows): FZ_P adjacent doubles
#if FZ_FLAGS & (1073741824u | 2147483648u)   /* FZ_VF_LANE_PAIRS / _SINGLES (named below): the lane's doubles in groups 64 x group size apart */
#define FZ_LG64 ((FZ_FLAGS & 1073741824u) ? 2 : 1)
__device__ __forceinline__ VD fz_ld_row64(const float* row, unsigned off)
{
   VD v;
#pragma unroll
   for (int g = 0; g < FZ_P / FZ_LG64; ++g)
#pragma unroll
      for (int j = 0; j < FZ_LG64; ++j) v[g * FZ_LG64 + j] = reinterpret_cast<const double*>(row)[off + (unsigned)(g * 64 * FZ_LG64 + j)];
   return v;
}
__device__ __forceinline__ void fz_st_row64(float* row, unsigned off, VD v)
{
#pragma unroll
   for (int g = 0; g < FZ_P / FZ_LG64; ++g)
#pragma unroll
      for (int j = 0; j < FZ_LG64; ++j) reinterpret_cast<double*>(row)[off + (unsigned)(g * 64 * FZ_LG64 + j)] = v[g * FZ_LG64 + j];
}
#else
__device__ __forceinline__ VD fz_ld_row64(const float* row, unsigned off) { return *reinterpret_cast<const VD*>(reinterpret_cast<const double*>(row) + off); }
__device__ __forceinline__ void fz_st_row64(float* row, unsigned off, VD v) { *reinterpret_cast<VD*>(reinterpret_cast<double*>(row) + off) = v; }
#endif

__device__ __forceinline__ double fz_get(double q, int) { return q; }
__device__ __forceinline__ double fz_get(fz_d2 q, int j) { return q[j]; }
__device__ __forceinline__ double fz_get(fz_d4 q, int j) { return q[j]; }

// output wires: float32 frames, or (FZ_VF_OUT_F64) float64 frames that keep the C++ double results of
// graphs with double literals un-narrowed (the tuple<double> of flowz.hpp:585-644 / tests.cpp:201)
#if FZ_FLAGS & FZ_VF_OUT_F64
typedef VD VO;
#define FZ_OUTW 2
__device__ __forceinline__ void fz_pack_out(float* fo, int k, double v)
{
   const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
   fo[2 * k] = __builtin_bit_cast(float, (unsigned)b);
   fo[2 * k + 1] = __builtin_bit_cast(float, (unsigned)(b >> 32));
}
#else
typedef V VO;
#define FZ_OUTW 1
__device__ __forceinline__ void fz_pack_out(float* fo, int k, float v) { fo[k] = v; }
#endif

#if FZ_PAIRS && (FZ_P < 2 * FZ_LG || (FZ_FLAGS & (FZ_VF_STREAM_MAJOR | FZ_VF_RAGGED)) || FZ_NFR > 0 || FZ_NFW > 0)
#error "lane groups: the frame kernel with two or four streams per lane, whole waves, no delay lines in HBM rings"
#endif
#if FZ_SKEW && (FZ_P != 1 || FZ_NIN != 1 || FZ_NOUT != 1)
#error "stage packing needs one stream per lane and a 1-in/1-out graph"
#endif


// Frame I/O goes through buffer instructions: the 128-bit resource (row base pointer + row size)
// is wave-uniform and lives in SGPRs, the lane's byte offset inside the row is ONE 32-bit VGPR
// that never changes, so stepping through time costs scalar adds only (no per-lane 64-bit address
// arithmetic on the VALU, which is the scarce unit here).  aux = 2 is the non-temporal hint.
// Cache policy of the frame accesses (gfx940+ cpol bits: sc0 = 1, nt = 2, sc1 = 16).  Loads: nt
// (streamed once).  Stores: nt | sc1 -- system-scope write-through keeps the output rows from
// lingering in L2 as dirty lines (measured +2 % at 1 M streams; the stage-packed kernel for few
// streams does best with sc1 alone, +1.2 %: profiles/r01/sweep_cache_policies.txt).
// Kernel experiments (FLOWZ_HIP_EXTRA_OPTS): -DFZ_DBG_NO_NT plain loads and stores; -DFZ_DBG_AUX_LD=<cpol> / -DFZ_DBG_AUX_ST=<cpol> another policy.
// A lane's output slice that leaves in MORE THAN ONE store (typed frames with four streams per lane: 32 bytes = two b128; three output
// wires: three dwords) must not be written through: each store covers only part of every 32-byte sector, and under nt | sc1 every part
// goes to HBM by itself -- PMC WRITE_SIZE 2.0 x the algorithmic bytes, 29-32 ms per block where plain write-back stores (L2 merges the
// parts) take 9.4 ms (round 4, profiles/r04/typed_frames_store_policy.txt).  Frame kernels only: the stream-major bodies write whole runs.
// Rows off the store grid (FZ_VF_ST_MERGE, set by finalize_variant from the row size; FZ_VF_RAGGED implies it) have the same trouble at the
// ends of every wave's footprint: its first and last 32-byte sectors are shared with the neighbouring waves, and written through
// (sc1) each half goes to HBM by itself.  nt alone lets L2 merge them: 1 000 001 streams 5.90 ms against 6.94 ms with nt | sc1 and
// 6.04 ms with plain stores; on rows ON the grid nt | sc1 stays ahead (5.47 / 5.64 ms; profiles/r04/rows_off_the_grid_store_policy.txt).
// widest vector access that keeps every piece naturally aligned (lane base = group * W floats)
#define FZ_VW(W) (((W) % 4 == 0) ? 4 : ((W) % 2 == 0) ? 2 : 1)
#define FZ_ST_W (FZ_LG * FZ_NOUT * FZ_OUTW)     /* floats of one contiguous piece of a lane's output slice */
#define FZ_ST_PIECES (FZ_ST_W / FZ_VW(FZ_ST_W))
#ifdef FZ_DBG_NO_NT
#define FZ_AUX_LD_DEFAULT 0
#define FZ_AUX_ST_DEFAULT 0
#else
#define FZ_AUX_LD_DEFAULT 2
#define FZ_AUX_ST_DEFAULT ((FZ_ST_PIECES > 1 && !(FZ_FLAGS & FZ_VF_STREAM_MAJOR)) ? 0 : (FZ_FLAGS & (FZ_VF_RAGGED | FZ_VF_ST_MERGE)) ? 2 : (FZ_SKEW ? 16 : 18))
#endif
#ifdef FZ_DBG_AUX_LD
#define FZ_AUX_LD (FZ_DBG_AUX_LD)
#else
#define FZ_AUX_LD FZ_AUX_LD_DEFAULT
#endif
#ifdef FZ_DBG_AUX_ST
#define FZ_AUX_ST (FZ_DBG_AUX_ST)
#else
#define FZ_AUX_ST FZ_AUX_ST_DEFAULT
#endif
#define FZ_SRD_FLAGS 0x00020000

typedef __amdgpu_buffer_rsrc_t fz_rsrc;

__device__ __forceinline__ fz_rsrc fz_make_rsrc(const float* base, unsigned bytes)
{
   return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), (short)0, (int)bytes, FZ_SRD_FLAGS);
}

// Loads take the row offset of a chunk in the instruction's SCALAR offset.  Stores do NOT: their row
// offset is added to the vector offset (loop-invariant VGPRs).  A buffer store whose data registers are
// overwritten by the next VALU instruction needs a wait state; with an SGPR soffset the compiler emits
// none (the GCN3/Vega ISA manual says none is needed then), but on gfx950 the last quarter of every 16
// lanes then stores the NEW register contents -- seen with b128 and with b64 stores (typed-graph fuzz
// test: frames of 3 x b128 / 5 x b64 per lane, lanes 12..15 and 28..31 wrong at a few time steps).
template <int VW> struct fz_buf;
template <> struct fz_buf<1> {
   typedef float T;
   static __device__ __forceinline__ T ld(fz_rsrc r, unsigned off, unsigned soff = 0) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)off, (int)soff, FZ_AUX_LD)); }
   static __device__ __forceinline__ void st(fz_rsrc r, unsigned off, T v, unsigned soff = 0) { __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, (int)(off + soff), 0, FZ_AUX_ST); }
   static __device__ __forceinline__ T ld0(fz_rsrc r, unsigned off) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0)); }   // plain cache policy
   static __device__ __forceinline__ void st0(fz_rsrc r, unsigned off, T v) { __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, (int)off, 0, 0); }
};
template <> struct fz_buf<2> {
   typedef fz_f2 T;
   static __device__ __forceinline__ T ld(fz_rsrc r, unsigned off, unsigned soff = 0) { return __builtin_bit_cast(fz_f2, __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, (int)soff, FZ_AUX_LD)); }
   static __device__ __forceinline__ void st(fz_rsrc r, unsigned off, T v, unsigned soff = 0) { __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(fz_u2, v), r, (int)(off + soff), 0, FZ_AUX_ST); }
   static __device__ __forceinline__ T ld0(fz_rsrc r, unsigned off) { return __builtin_bit_cast(fz_f2, __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0)); }
   static __device__ __forceinline__ void st0(fz_rsrc r, unsigned off, T v) { __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(fz_u2, v), r, (int)off, 0, 0); }
};
template <> struct fz_buf<4> {
   typedef fz_f4 T;
   static __device__ __forceinline__ T ld(fz_rsrc r, unsigned off, unsigned soff = 0) { return __builtin_bit_cast(fz_f4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, (int)soff, FZ_AUX_LD)); }
   static __device__ __forceinline__ void st(fz_rsrc r, unsigned off, T v, unsigned soff = 0) { __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(fz_u4, v), r, (int)(off + soff), 0, FZ_AUX_ST); }
   static __device__ __forceinline__ T ld0(fz_rsrc r, unsigned off) { return __builtin_bit_cast(fz_f4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0)); }
   static __device__ __forceinline__ void st0(fz_rsrc r, unsigned off, T v) { __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(fz_u4, v), r, (int)off, 0, 0); }
};

__device__ __forceinline__ float fz_get(float q, int) { return q; }
__device__ __forceinline__ float fz_get(fz_f2 q, int j) { return q[j]; }
__device__ __forceinline__ float fz_get(fz_f4 q, int j) { return q[j]; }
__device__ __forceinline__ void fz_set(float& q, int, float v) { q = v; }
__device__ __forceinline__ void fz_set(fz_f2& q, int j, float v) { q[j] = v; }
__device__ __forceinline__ void fz_set(fz_f4& q, int j, float v) { q[j] = v; }

// one lane's frame slice: W contiguous floats starting `boff` bytes into the row described by r
// (soff: a wave-uniform byte offset added by the instruction itself -- the row inside a chunk)
template <int W> __device__ __forceinline__ void fz_load_frame(fz_rsrc r, unsigned boff, float (&f)[W], unsigned soff = 0)
{
   constexpr int VW = FZ_VW(W);
#pragma unroll
   for (int k = 0; k < W / VW; ++k) {
      const typename fz_buf<VW>::T q = fz_buf<VW>::ld(r, boff + (unsigned)(k * VW * 4), soff);
#pragma unroll
      for (int j = 0; j < VW; ++j) f[k * VW + j] = fz_get(q, j);
   }
}

template <int W> __device__ __forceinline__ void fz_store_frame(fz_rsrc r, unsigned boff, const float (&f)[W], unsigned soff = 0)
{
   constexpr int VW = FZ_VW(W);
#pragma unroll
   for (int k = 0; k < W / VW; ++k) {
      typename fz_buf<VW>::T q;
#pragma unroll
      for (int j = 0; j < VW; ++j) fz_set(q, j, f[k * VW + j]);
      fz_buf<VW>::st(r, boff + (unsigned)(k * VW * 4), q, soff);
   }
}

// a lane's slice of a frame row: W floats -- contiguous, or (FZ_PAIRS) two halves 128 streams apart
template <int W> __device__ __forceinline__ void fz_load_lane(fz_rsrc r, unsigned boff, float (&f)[W], unsigned soff = 0)
{
#if FZ_PAIRS
   constexpr int WG = W / FZ_NGRP;                          // floats of one group's slice (0: a graph without input wires, W is a placeholder)
   if constexpr (WG > 0) {
#pragma unroll
      for (int g = 0; g < FZ_NGRP; ++g) {
         float part[WG];
         fz_load_frame<WG>(r, boff + (unsigned)g * 64u * (unsigned)WG * 4u, part, soff);
#pragma unroll
         for (int k = 0; k < WG; ++k) f[g * WG + k] = part[k];
      }
   }
#else
   fz_load_frame<W>(r, boff, f, soff);
#endif
}
template <int W> __device__ __forceinline__ void fz_store_lane(fz_rsrc r, unsigned boff, const float (&f)[W], unsigned soff = 0)
{
#if FZ_PAIRS
   constexpr int WG = W / FZ_NGRP;
   if constexpr (WG > 0) {
#pragma unroll
      for (int g = 0; g < FZ_NGRP; ++g) {
         float part[WG];
#pragma unroll
         for (int k = 0; k < WG; ++k) part[k] = f[g * WG + k];
         fz_store_frame<WG>(r, boff + (unsigned)g * 64u * (unsigned)WG * 4u, part, soff);
      }
   }
#else
   fz_store_frame<W>(r, boff, f, soff);
#endif
}

// planar per-stream rows (state, params): FZ_P adjacent floats of one row of ns floats.
// Through buffer descriptors of exactly one row (round 4): the row's base is wave-uniform (scalar registers) and the lane's offset is
// ONE 32-bit register shared by all rows.  With plain pointers the compiler computed a 64-bit vector address per row and kept all of
// them alive from the state load at the start of a block to the state store at its end -- 28 of the 128 registers a lane of the
// four-streams-per-lane headline kernel has (seen in the ISA: v_lshl_add_u64 x 14 in the prologue, global_store_dwordx4 through the
// same register pairs in the epilogue).  A side effect: FZ_VF_RAGGED needs nothing more -- the dwords of the last lane that lie past
// the end of a row read as zero and are not written (raw buffers are range-checked per dword), and rows of an odd stream count,
// which are only 4-byte aligned, are fine for b64 / b128 buffer accesses.
#if FZ_PAIRS
__device__ __forceinline__ V fz_ld_row(const float* row, unsigned off, size_t ns)
{
   const fz_rsrc r = fz_make_rsrc(row, (unsigned)ns * 4u);
   V v;
#pragma unroll
   for (int g = 0; g < FZ_NGRP; ++g) {
      const typename fz_buf<FZ_LG>::T q = fz_buf<FZ_LG>::ld0(r, (off + (unsigned)g * 64u * FZ_LG) * 4u);
#pragma unroll
      for (int j = 0; j < FZ_LG; ++j) v[g * FZ_LG + j] = fz_get(q, j);
   }
   return v;
}
__device__ __forceinline__ void fz_st_row(float* row, unsigned off, size_t ns, V v)
{
   const fz_rsrc r = fz_make_rsrc(row, (unsigned)ns * 4u);
#pragma unroll
   for (int g = 0; g < FZ_NGRP; ++g) {
      typename fz_buf<FZ_LG>::T q;
#pragma unroll
      for (int j = 0; j < FZ_LG; ++j) fz_set(q, j, v[g * FZ_LG + j]);
      fz_buf<FZ_LG>::st0(r, (off + (unsigned)g * 64u * FZ_LG) * 4u, q);
   }
}
#else
__device__ __forceinline__ V fz_ld_row(const float* row, unsigned off, size_t ns) { return fz_buf<FZ_P>::ld0(fz_make_rsrc(row, (unsigned)ns * 4u), off * 4u); }
__device__ __forceinline__ void fz_st_row(float* row, unsigned off, size_t ns, V v) { fz_buf<FZ_P>::st0(fz_make_rsrc(row, (unsigned)ns * 4u), off * 4u, v); }
#endif
// (one float of a row: the stage-packed bodies, one stream per lane)
__device__ __forceinline__ float fz_ld_f(const float* row, unsigned off, size_t ns) { return fz_buf<1>::ld0(fz_make_rsrc(row, (unsigned)ns * 4u), off * 4u); }
__device__ __forceinline__ void fz_st_f(float* row, unsigned off, size_t ns, float v) { fz_buf<1>::st0(fz_make_rsrc(row, (unsigned)ns * 4u), off * 4u, v); }

// a value that is the same in every lane, as the compiler should keep it: in a scalar register (an operand of the packed
// instructions that use it, not a vector register per use)
__device__ __forceinline__ float fz_uniform_f(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }

struct fz_args {
   const float* in;
   float* out;
   float* state;
   const float* params;
   const float* mod;                           // sample-rate modulators [n_mod][mod_stride] (fz_program_set_modulation)
   unsigned int* sync;                         // FZ_VF_GRID_SYNC: one arrival counter per (generation, XCD), 128 bytes apart, zeroed before the launch
   unsigned long long n_streams;
   unsigned int n_samples;
   unsigned int n_groups;                      // n_streams / FZ_P lanes of work
   unsigned int tile_streams;                  // streams per frame tile (== n_streams: plain time-major)
   unsigned int tile_blocks;                   // workgroups per tile = tile_streams / (FZ_P * FZ_BLOCK), 0 when untiled
   unsigned int rows_total;                    // samples the frame buffers hold per tile (>= row0 + n_samples)
   unsigned int row0;                          // first sample of this block inside the buffers
   unsigned int mod_stride;
   unsigned int n_blocks;                      // blocks of work of the whole call (a lap's launch covers part of them)
   unsigned int group0;                        // a launch that covers PART of the streams (one lap of a block, or the remainder behind the laps): its
                                               // lanes take on stream groups group0, group0 + 1, ... (n_groups: where they end, n_streams: the rows' pitch)
   unsigned int reserved0;
   float c[FZ_NCONST > 0 ? FZ_NCONST : 1];     // uniform coefficients (literal terminals)
   double cd[FZ_NCONST64 > 0 ? FZ_NCONST64 : 1];   // float64 literal terminals
};

// slot of a ring of S slots (S not a power of two) for position `pos`, which is a sample index minus a delay of at most S: the
// caller's unsigned arithmetic may have wrapped below zero -- a position within S of 2^32 is such a wrap (no block has that many samples)
template <unsigned S> __device__ __forceinline__ unsigned fz_ring_mod(unsigned pos) { return (pos >= 0u - S ? pos + S : pos) % S; }   // (wave-uniform: scalar instructions)

#if FZ_LDS_SLOTS > 0
#define FZ_RING_DECL __shared__ V fz_ring[FZ_LDS_SLOTS * FZ_BLOCK];
#define FZ_RING fz_ring
#else
#define FZ_RING_DECL
#define FZ_RING ((V*)nullptr)
#endif

// LDS rings vectorised in time (FZ_RING_G > 0): entry e of a run of 16-byte vectors that hold 4 / FZ_P consecutive slots each -- with
// the constant e of an unrolled step a register (pair) of the run, no instruction
#if FZ_P == 1
__device__ __forceinline__ V fz_ring_pick(const fz_f4* a, int e) { return a[e >> 2][e & 3]; }
__device__ __forceinline__ void fz_ring_put(fz_f4* a, int e, V v) { a[e >> 2][e & 3] = v; }
#elif FZ_P == 2
__device__ __forceinline__ V fz_ring_pick(const fz_f4* a, int e) { const fz_f4 q = a[e >> 1]; return (e & 1) ? (V){q[2], q[3]} : (V){q[0], q[1]}; }
__device__ __forceinline__ void fz_ring_put(fz_f4* a, int e, V v)
{
   if (e & 1) { a[e >> 1][2] = v[0]; a[e >> 1][3] = v[1]; }
   else { a[e >> 1][0] = v[0]; a[e >> 1][1] = v[1]; }
}
#else
__device__ __forceinline__ V fz_ring_pick(const fz_f4* a, int e) { return a[e]; }
__device__ __forceinline__ void fz_ring_put(fz_f4* a, int e, V v) { a[e] = v; }
#endif

#include "fz_graph_body.h"     // generated: struct fz_graph { load_state, load_params, step, store_state }

#define FZ_WIN (FZ_P * FZ_NIN)
#define FZ_WOUT (FZ_P * FZ_NOUT * FZ_OUTW)      // floats of one lane's output frame slice
#define FZ_WIN1 (FZ_WIN > 0 ? FZ_WIN : 1)

// FZ_MINWAVES (variant flags bits 8..11): ask the register allocator for at least that many waves
// per SIMD (0 = let it use what it wants)
#if FZ_MINWAVES > 0
#define FZ_BOUNDS __launch_bounds__(FZ_BLOCK, FZ_MINWAVES)
#else
#define FZ_BOUNDS __launch_bounds__(FZ_BLOCK)
#endif

// ONE of the three bodies follows, chosen by the library from the variant's flags when it assembles the source (fz_codegen.cpp:
// skeleton_source): a kernel's text -- and with it the name of its code object in the kernel cache -- holds only the body it runs
//@body sm_common fz_kernel_sm_common.hip.inc
//@body sm_pair fz_kernel_sm_pair.hip.inc
//@body sm_long fz_kernel_sm_long.hip.inc
//@body sm_short fz_kernel_sm_short.hip.inc
//@body wave_split fz_kernel_wave_split.hip.inc
//@body frames fz_kernel_frames.hip.inc
