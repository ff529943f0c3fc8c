// fz_pcm16_sm_kernel -- hand-written gfx950 (MI355X, CDNA4) walk over STREAM-MAJOR buffers whose frames are 16-bit PCM on one side or
// on both (include/flowz_hip.h: fz_run_block_pcm16_stream_major).  It follows the common head of fz_block_kernel.hip.inc (the types,
// the generated body) the way fz_kernel_pcm16.hip.inc does, and is a kernel text of its own: no other kernel's source holds a line of it.
//
// The arithmetic is the generated fz_graph::step of the frame kernels, unchanged: between the two conversions the block is
// fz_run_block_stream_major, bit for bit.  The conversions (the rule is stated once, in include/flowz_hip.h; restated here because
// sharing the two functions would change the time-major PCM kernel's source):
//   in   x = (float)q * 2^-15                                   exact
//   out  r = y * 32768.0f;  NaN -> 0;  r >= 32767 -> 32767;  r <= -32768 -> -32768;  else round to nearest, ties to even
//
// Buffers: in [n_streams][rows_total][n_in], out [n_streams][rows_total][n_out], each side int16 or float32 (flags bit 0: `in` is
// int16, bit 1: `out` is int16); the block is the window of rows [row0, row0 + n_samples).  State, per-stream coefficients and uniform
// coefficients exactly as for fz_run_block ([row][n_streams]).
//
// Schedule (the plain one of fz_kernel_sm_short.hip.inc and fz_kernel_adjoint_sm.hip.inc): one stream per lane, ONE wave per workgroup.
// The 64 lanes fetch a chunk [64 streams][FZ_U rows] as 16-byte PIECES laid along the rows -- 8 int16 samples or 4 floats; consecutive
// lanes take consecutive pieces of one stream's run --, park them in the wave's LDS patch, and every lane walks its own patch row in
// a real loop of FZ_PS_G unrolled steps: the chunk lives in the patch, not in registers.  Outputs are written into the patch row and
// leave the same way in reverse.  A patch row is [in part: FZ_U x n_in samples][out part: FZ_U x n_out samples][16 bytes of padding]:
// the parts are apart because a step with int16 in and float32 out writes more bytes than it reads.  Patch bytes per wave:
// 64 x (FZ_U x (n_in x ie + n_out x oe) + 16), ie / oe = 2 or 4 (fz_pcm16.cpp: pcm16_sm_chunk_rows chooses FZ_U).
//
// Prefetch: the first FZ_PS_HOLD pieces a lane owes to the NEXT chunk are requested before the current chunk's steps and held in
// registers across them; they are parked once the steps are done, and the pieces behind them are fetched then, FZ_PS_FLIGHT at a time
// (every piece of a wide float32 in-run in flight at once would pass the register file).
//
// Edges, without a workgroup barrier (fz_ps_wave_sync orders the wave's own LDS traffic):
//   * the last wave's missing streams: their lanes shadow the wave's last stream (its run, its state) and store nothing; pieces of
//     missing streams are fetched from the wave's last stream (no branch per piece) and never stored;
//   * only whole chunks travel as pieces, so no piece reaches outside the window; the rows behind the last whole chunk run one step
//     at a time, every lane on its own run, with 2-byte accesses on an int16 side: rows outside the window are never touched;
//   * in place (in == out, int16 both sides, n_in == n_out): a chunk's out-run leaves after the NEXT chunk's held pieces were
//     requested -- other rows --, and after its own in-run was parked.
#define FZ_VF_PCM16_SM 8192u
#define FZ_PS_IN ((FZ_FLAGS & 1u) != 0)
#define FZ_PS_OUT ((FZ_FLAGS & 2u) != 0)
#if FZ_P != 1 || FZ_BLOCK != 64 || (FZ_U % 8) != 0 || FZ_SKEW || FZ_LDS_SLOTS > 0 || FZ_NFR > 0 || FZ_NFW > 0 || FZ_NMOD > 0 || FZ_NCONST64 > 0 || (FZ_FLAGS & FZ_VF_OUT_F64)
#error "stream-major PCM frames: one stream per lane, one wave per workgroup, chunks of whole int16 pieces, a float32 graph whose delay lines live in registers"
#endif
#if !(FZ_FLAGS & 3u) || !(FZ_FLAGS & FZ_VF_PCM16_SM)
#error "stream-major PCM frames: one side at least is int16 (float32 on both is the stream-major kernel)"
#endif

#define FZ_PS_A(n) ((n) > 0 ? (n) : 1)
#define FZ_PS_IE (FZ_PS_IN ? 2 : 4)                       /* bytes per sample */
#define FZ_PS_OE (FZ_PS_OUT ? 2 : 4)
#define FZ_PS_IB (FZ_U * FZ_NIN * FZ_PS_IE)               /* bytes of one stream's in-run of a chunk: the in part of a patch row */
#define FZ_PS_OB (FZ_U * FZ_NOUT * FZ_PS_OE)              /* ... of its out-run: the out part, behind it */
#define FZ_PS_ROW (FZ_PS_IB + FZ_PS_OB + 16)              /* padded patch row */
#define FZ_PS_PI (FZ_PS_IB / 16)                          /* pieces per stream and chunk = pieces per lane and chunk */
#define FZ_PS_PO (FZ_PS_OB / 16)
#define FZ_PS_G 8                                         /* rows per trip of the step loop: 8 x wires samples are whole pieces */
#define FZ_PS_GI (FZ_PS_G * FZ_NIN * FZ_PS_IE / 4)        /* dwords of a trip's frames */
#define FZ_PS_GO (FZ_PS_G * FZ_NOUT * FZ_PS_OE / 4)
#define FZ_PS_HOLD (FZ_PS_PI < 16 ? FZ_PS_PI : 16)        /* pieces of the next chunk held in registers across a chunk's steps */
#define FZ_PS_FLIGHT 8                                    /* pieces in flight at once behind them */

struct fz_pcm_sm_args {
   const void* in;             // [n_streams][rows_total][n_in]   int16 or float32
   void* out;                  // [n_streams][rows_total][n_out]  int16 or float32
   float* state;               // [n_state][n_streams]
   const float* params;        // [n_param][n_streams]
   unsigned long long n_streams;
   unsigned int n_samples;
   unsigned int rows_total;
   unsigned int row0;
   unsigned int reserved0;
   float c[FZ_PS_A(FZ_NCONST)];
};

__device__ __forceinline__ void fz_ps_wave_sync()
{
   __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
   __builtin_amdgcn_wave_barrier();
   __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float fz_ps_to_float(int q) { return (float)q * 0x1p-15f; }
__device__ __forceinline__ int fz_ps_from_float(float y)
{
   const float r = y * 32768.0f;
   return r != r ? 0 : r >= 32767.0f ? 32767 : r <= -32768.0f ? -32768 : (int)__builtin_rintf(r);
}

// Piece e = i * 64 + lane of a chunk's part is piece e % PIECES of patch row e / PIECES: 16 bytes at byte 16 * (e % PIECES) of that
// stream's run.  `rows` streams of the wave exist.  global -> registers: pieces [FIRST, FIRST + N) of the lane; `g` the first byte of
// the wave's first run, `gstride` bytes from one stream's run to the next.
template <int PIECES, int FIRST, int N>
__device__ __forceinline__ void fz_ps_request(fz_u4 (&h)[FZ_PS_A(N)], const char* g, size_t gstride, unsigned rows, unsigned lane)
{
   constexpr unsigned PP = PIECES > 0 ? PIECES : 1;
#pragma unroll
   for (int i = 0; i < N; ++i) {
      const unsigned e = (unsigned)(FIRST + i) * 64u + lane, row = e / PP, q = e % PP;
      const unsigned grow = row < rows ? row : rows - 1u;
      h[i] = __builtin_nontemporal_load(reinterpret_cast<const fz_u4*>(g + grow * gstride + q * 16u));
   }
}
// registers -> the in part of the patch
template <int PIECES, int FIRST, int N>
__device__ __forceinline__ void fz_ps_park(unsigned char* patch, const fz_u4 (&h)[FZ_PS_A(N)], unsigned lane)
{
   constexpr unsigned PP = PIECES > 0 ? PIECES : 1;
#pragma unroll
   for (int i = 0; i < N; ++i) {
      const unsigned e = (unsigned)(FIRST + i) * 64u + lane, row = e / PP, q = e % PP;
      *reinterpret_cast<fz_u4*>(patch + row * FZ_PS_ROW + q * 16u) = h[i];
   }
}
// pieces [FIRST, PIECES) of a chunk's in-run into the patch, FZ_PS_FLIGHT at a time
template <int PIECES, int FIRST>
__device__ __forceinline__ void fz_ps_fetch(unsigned char* patch, const char* g, size_t gstride, unsigned rows, unsigned lane)
{
   if constexpr (FIRST < PIECES) {
      constexpr int N = PIECES - FIRST < FZ_PS_FLIGHT ? PIECES - FIRST : FZ_PS_FLIGHT;
      fz_u4 h[N];
      fz_ps_request<PIECES, FIRST, N>(h, g, gstride, rows, lane);
      fz_ps_park<PIECES, FIRST, N>(patch, h, lane);
      asm volatile("" ::: "memory");                        // (parked before the next are requested)
      fz_ps_fetch<PIECES, FIRST + N>(patch, g, gstride, rows, lane);
   }
}
// the out part of the patch -> global: whole pieces of the streams that exist
template <int PIECES>
__device__ __forceinline__ void fz_ps_flush(const unsigned char* patch, char* g, size_t gstride, unsigned rows, unsigned lane)
{
   constexpr unsigned PP = PIECES > 0 ? PIECES : 1;
#pragma unroll
   for (int i = 0; i < PIECES; ++i) {
      const unsigned e = (unsigned)i * 64u + lane, row = e / PP, q = e % PP;
      if (row < rows)
         __builtin_nontemporal_store(*reinterpret_cast<const fz_u4*>(patch + row * FZ_PS_ROW + FZ_PS_IB + q * 16u),
                                     reinterpret_cast<fz_u4*>(g + row * gstride + q * 16u));
   }
}

// sample e of a trip's packed frames as the float the graph reads, and the way back
__device__ __forceinline__ float fz_ps_in_sample(const unsigned (&d)[FZ_PS_A(FZ_PS_GI)], int e)
{
#if FZ_PS_IN
   return fz_ps_to_float((short)(d[e >> 1] >> ((e & 1) * 16)));
#else
   return __builtin_bit_cast(float, d[e]);
#endif
}
__device__ __forceinline__ void fz_ps_out_sample(unsigned (&d)[FZ_PS_A(FZ_PS_GO)], int e, float y)
{
#if FZ_PS_OUT
   const unsigned q = (unsigned)fz_ps_from_float(y) & 0xFFFFu;
   d[e >> 1] = (e & 1) ? (d[e >> 1] | (q << 16)) : q;
#else
   d[e] = __builtin_bit_cast(unsigned, y);
#endif
}

extern "C" __global__ void __launch_bounds__(64) FZ_KERNEL(const fz_pcm_sm_args a)
{
   __shared__ __attribute__((aligned(16))) unsigned char fz_ps_patch[64 * FZ_PS_ROW];
   float fz_c[FZ_PS_A(FZ_NCONST)];
   double fz_cd[1] = {0.0};
#pragma unroll
   for (int k = 0; k < FZ_PS_A(FZ_NCONST); ++k) fz_c[k] = a.c[k];
   // the block order of the frame kernels: workgroups are dispatched round-robin over the 8 XCDs, each XCD takes one contiguous range
   // of waves (blockIdx.x & 7 is the XCD the workgroup sits on)
   unsigned blk = blockIdx.x;
   {
      const unsigned nb = gridDim.x, xcd = blk & 7u, idx = blk >> 3, q = nb >> 3, r = nb & 7u;
      blk = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + idx;
   }
   const size_t ns = (size_t)a.n_streams;
   const unsigned lane = threadIdx.x;
   const size_t s_base = (size_t)blk * 64u;                  // first stream of this wave (the grid holds no wave past the last stream)
   const unsigned rows_here = (unsigned)(ns - s_base < 64u ? ns - s_base : 64u);
   const bool active = lane < rows_here;
   const unsigned prow = active ? lane : rows_here - 1u;     // idle lanes shadow the wave's last stream, store nothing
   const unsigned s = (unsigned)s_base + prow;               // (< 2^30: the host checks)
   const unsigned T = a.n_samples;
   unsigned char* const mine = fz_ps_patch + prow * FZ_PS_ROW;
   // the wave's first run of each buffer: stream s_base, row row0; and this lane's own runs
   const size_t istride = (size_t)a.rows_total * (FZ_NIN * FZ_PS_IE), ostride = (size_t)a.rows_total * (FZ_NOUT * FZ_PS_OE);
   const char* const gin = static_cast<const char*>(a.in) + s_base * istride + (size_t)a.row0 * (FZ_NIN * FZ_PS_IE);
   char* const gout = static_cast<char*>(a.out) + s_base * ostride + (size_t)a.row0 * (FZ_NOUT * FZ_PS_OE);

   fz_graph G;
   const unsigned ph[1] = {0};
   G.load_params(a.params, ns, s);
   G.load_state(a.state, ns, s, (V*)nullptr, lane, ph);

#define FZ_PS_STEP(xs, ys, tt)                                                                                \
   {                                                                                                          \
      V hr[1], hw[1];                                                                                         \
      G.step(xs, ys, fz_c, fz_cd, (V*)nullptr, lane, (tt), hr, hw, (const float*)nullptr, 0u, -1);            \
   }

   const unsigned nchunks = T / FZ_U;
   if (nchunks) fz_ps_fetch<FZ_PS_PI, 0>(fz_ps_patch, gin, istride, rows_here, lane);
   for (unsigned c = 0; c < nchunks; ++c) {
      const bool more = c + 1u < nchunks;                    // (wave-uniform)
      const char* const gnext = gin + (size_t)(c + 1u) * FZ_PS_IB;
      fz_u4 hold[FZ_PS_A(FZ_PS_HOLD)];
      if (more) fz_ps_request<FZ_PS_PI, 0, FZ_PS_HOLD>(hold, gnext, istride, rows_here, lane);
      fz_ps_wave_sync();                                     // the chunk's in-run is parked; the out-run before it has left
#pragma unroll 1
      for (unsigned u0 = 0; u0 < FZ_U; u0 += FZ_PS_G) {
         unsigned xi[FZ_PS_A(FZ_PS_GI)], yo[FZ_PS_A(FZ_PS_GO)];
         xi[0] = 0u;
         yo[0] = 0u;
#pragma unroll
         for (int k = 0; k < FZ_PS_GI / 4; ++k) {
            const fz_u4 q = *reinterpret_cast<const fz_u4*>(mine + u0 * (FZ_NIN * FZ_PS_IE) + k * 16);
            xi[4 * k] = q[0];
            xi[4 * k + 1] = q[1];
            xi[4 * k + 2] = q[2];
            xi[4 * k + 3] = q[3];
         }
#pragma unroll
         for (int j = 0; j < FZ_PS_G; ++j) {
            V x[FZ_PS_A(FZ_NIN)];
            VO y[FZ_PS_A(FZ_NOUT)];
            x[0] = 0.f;
#pragma unroll
            for (int w = 0; w < FZ_NIN; ++w) x[w] = fz_ps_in_sample(xi, j * FZ_NIN + w);
            FZ_PS_STEP(x, y, c * FZ_U + u0 + (unsigned)j)
#pragma unroll
            for (int w = 0; w < FZ_NOUT; ++w) fz_ps_out_sample(yo, j * FZ_NOUT + w, y[w]);
         }
         if (active) {
#pragma unroll
            for (int k = 0; k < FZ_PS_GO / 4; ++k)
               *reinterpret_cast<fz_u4*>(mine + FZ_PS_IB + u0 * (FZ_NOUT * FZ_PS_OE) + k * 16) = (fz_u4){yo[4 * k], yo[4 * k + 1], yo[4 * k + 2], yo[4 * k + 3]};
         }
      }
      fz_ps_wave_sync();                                     // every lane is done with its in part and has written its out part
      fz_ps_flush<FZ_PS_PO>(fz_ps_patch, gout + (size_t)c * FZ_PS_OB, ostride, rows_here, lane);
      if (more) {
         fz_ps_park<FZ_PS_PI, 0, FZ_PS_HOLD>(fz_ps_patch, hold, lane);
         fz_ps_fetch<FZ_PS_PI, FZ_PS_HOLD>(fz_ps_patch, gnext, istride, rows_here, lane);
      }
   }
   // the rows behind the last whole chunk, one at a time, every lane on its own run
   {
      const char* const li = gin + (size_t)prow * istride;
      char* const lo = gout + (size_t)prow * ostride;
      for (unsigned t = nchunks * FZ_U; t < T; ++t) {
         V x[FZ_PS_A(FZ_NIN)];
         VO y[FZ_PS_A(FZ_NOUT)];
         x[0] = 0.f;
#pragma unroll
         for (int w = 0; w < FZ_NIN; ++w) {
#if FZ_PS_IN
            x[w] = fz_ps_to_float(reinterpret_cast<const short*>(li)[(size_t)t * FZ_NIN + w]);
#else
            x[w] = reinterpret_cast<const float*>(li)[(size_t)t * FZ_NIN + w];
#endif
         }
         FZ_PS_STEP(x, y, t)
         if (active) {
#pragma unroll
            for (int w = 0; w < FZ_NOUT; ++w) {
#if FZ_PS_OUT
               reinterpret_cast<short*>(lo)[(size_t)t * FZ_NOUT + w] = (short)fz_ps_from_float(y[w]);
#else
               reinterpret_cast<float*>(lo)[(size_t)t * FZ_NOUT + w] = y[w];
#endif
            }
         }
      }
   }

   if (active) G.store_state(a.state, ns, s, (V*)nullptr, lane, T);
}
