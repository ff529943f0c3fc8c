// Part of fz_block_kernel.hip.inc (inlined by embed.py): what the kernel bodies for STREAM-MAJOR buffers [stream][t][wire] share.
// fz_codegen.cpp (skeleton_source) puts it between the common head and the ONE stream-major body a kernel runs: the pair long-run
// body (fz_kernel_sm_pair.hip.inc), the one-stream long-run body (fz_kernel_sm_long.hip.inc) or the short-chunk body
// (fz_kernel_sm_short.hip.inc).
// =====================================================================================================
// Stream-major frames: in [n_streams][rows_total][n_in], out [n_streams][rows_total][n_out] -- one
// contiguous buffer per stream, the way every closure of the reference consumes its samples
// (test/benchmark.cpp:137-147).  A lane still owns one stream, but a lane-per-row load would touch one
// cache line per lane; instead the 64 lanes of a wave fetch the chunk [64 streams][FZ_U samples] as
// float4 pieces laid along the rows (8 lanes cover one stream's 128 B when FZ_U * n_in = 32), park them
// in a wave-private LDS patch and read their own row back: the transposition costs two LDS passes per
// chunk and no extra HBM traffic.  Outputs go the same way in reverse.  One stream per lane, no stage
// packing, delays up to the LDS rings.
// =====================================================================================================
#if FZ_P > 2 || FZ_NFR > 0 || FZ_NFW > 0 || (FZ_FLAGS & FZ_VF_OUT_F64) || (FZ_U % 4) != 0
#error "stream-major frames: one or two streams per lane, unroll % 4 == 0, no far delay lines / float64 frames"
#endif
#if FZ_SKEW && FZ_U <= FZ_SKEW
#error "stage-packed stream-major frames: the chunk must be longer than the skew"
#endif
#define FZ_SM_CI (FZ_U * FZ_NIN)                       /* floats per stream per chunk */
#define FZ_SM_CO (FZ_U * FZ_NOUT)
#define FZ_SM_CW (FZ_SM_CI > FZ_SM_CO ? FZ_SM_CI : FZ_SM_CO)
#define FZ_SM_ROW (FZ_SM_CW + 4)                       /* padded patch row: own-row b128 accesses hit 32 distinct banks */
#define FZ_SM_PI (FZ_SM_CI / 4)                        /* float4 pieces per stream */
#define FZ_SM_PO (FZ_SM_CO / 4)
#define FZ_SM_PI1 (FZ_SM_PI > 0 ? FZ_SM_PI : 1)
#define FZ_SM_SW (64 * FZ_P)                           /* streams of one wave */

__device__ __forceinline__ void fz_wave_sync()
{
   __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
   __builtin_amdgcn_wave_barrier();
   __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// (kernel experiments, FLOWZ_HIP_EXTRA_OPTS=-DFZ_DBG_NOLOAD / -DFZ_DBG_NOSTORE: the runs go through zero-byte descriptors --
//  the same instruction stream without the memory traffic)
#ifdef FZ_DBG_NOLOAD
constexpr bool fz_dbg_ld = false;
#else
constexpr bool fz_dbg_ld = true;
#endif
#ifdef FZ_DBG_NOSTORE
constexpr bool fz_dbg_st = false;
#else
constexpr bool fz_dbg_st = true;
#endif

// (kernel experiment, FLOWZ_HIP_EXTRA_OPTS=-DFZ_DBG_PHASE_CLOCKS: one wave in the middle of the grid sums the shader clocks it spends in
//  each of the n sections of its phases -- FZ_SM_CLK(k) closes section k, FZ_SM_CLK(0) only starts the clock -- and leaves the sums in
//  the first words of its first output row: wrong results, a profile of the phase.  Macros on purpose: with the clock as an object of a
//  class, empty without the switch, the long-run kernels came out with other machine code.)
#ifdef FZ_DBG_PHASE_CLOCKS
#define FZ_SM_CLK_DECL(n) unsigned long long clk_sum[n] = {}, clk_last = 0;
#define FZ_SM_CLK(k)                                                                     \
   {                                                                                     \
      unsigned long long now_;                                                           \
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now_)::"memory");   \
      if ((k) > 0) clk_sum[k] += now_ - clk_last;                                        \
      clk_last = now_;                                                                   \
   }
/* wait for the in-run: its loads are older than the `newer` vector-memory instructions issued since (the stores of the last out-run) */
#define FZ_SM_CLK_WAITLOADS(newer) asm volatile("s_waitcnt vmcnt(" #newer ")" ::: "memory");
#define FZ_SM_CLK_WRITE(n)                                                               \
   if (blockIdx.x == gridDim.x / 2u && tid == 0) {                                       \
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                   \
      for (int k = 0; k < (n); ++k) reinterpret_cast<unsigned*>(a.out)[k] = (unsigned)clk_sum[k];   \
   }
#else
#define FZ_SM_CLK_DECL(n)
#define FZ_SM_CLK(k)
#define FZ_SM_CLK_WAITLOADS(newer)
#define FZ_SM_CLK_WRITE(n)
#endif
