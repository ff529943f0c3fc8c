// fz_pcm16_kernel -- hand-written gfx950 (MI355X, CDNA4) frame walk for blocks whose frames are 16-bit PCM on one side or on both
// (include/flowz_hip.h: fz_run_block_pcm16).  It follows the common head of fz_block_kernel.hip.inc (the types, the buffer accessors,
// the generated body) the way the forward bodies do, and is a kernel text of its own: no forward kernel's source holds a line of it.
//
// The arithmetic is the generated fz_graph::step of the frame kernels, unchanged: between the two conversions the block is
// fz_run_block, bit for bit.  The conversions (the rule is stated once, in include/flowz_hip.h):
//   in   x = (float)q * 2^-15                                   exact
//   out  r = y * 32768.0f;  NaN -> 0;  r >= 32767 -> 32767;  r <= -32768 -> -32768;  else round to nearest, ties to even
//
// Frames are time-major [t][stream][wire], each side int16 or float32 (flags bit 0: `in` is int16, bit 1: `out` is int16); state,
// per-stream coefficients and uniform coefficients exactly as for fz_run_block.  One lane owns FZ_P adjacent streams for the whole
// block.  Every row goes through a wave-uniform descriptor of exactly that row (scalar registers) and the lane's byte offset inside a
// row is one register that never changes: what lies past the end of a row -- the missing streams of the last lane when the stream
// count is no multiple of FZ_P -- reads as zero and is not written.  Input rows are requested one chunk (FZ_U rows) ahead into two
// register buffers, still packed: an int16 row costs half the registers of a float row.
//
// ON the dword grid (flags bit 2 clear: every int16 row is a whole number of dwords) a lane's int16 slice is FZ_P * wires / 2 dwords,
// moved with the widest naturally aligned access: two streams of one wire are ONE dword -- a packed operand pair after conversion --,
// four are a b64 access and 512 bytes per wave and row.  OFF the grid (bit 2: streams x wires is odd on an int16 side, so every
// other row starts two bytes off) the int16 sides use 2-byte accesses, one per sample; float sides are on the grid always.
//
// Store policy, as fz_block_kernel.hip.inc states it for the frame kernels: written through (nt | sc1) only where a lane's slice leaves
// in ONE store and the rows start on the store grid (no FZ_VF_ST_MERGE), so that every instruction of a wave covers whole 32-byte
// sectors; rows off that grid leave with nt alone (L2 merges the sectors two waves share), slices of several stores -- the 2-byte
// stores among them -- with the plain policy.  Stores take no scalar offset (the note on buffer stores in the head).
#define FZ_PCM_IN ((FZ_FLAGS & 1u) != 0)
#define FZ_PCM_OUT ((FZ_FLAGS & 2u) != 0)
#define FZ_PCM_B16 ((FZ_FLAGS & 4u) != 0)
#if FZ_P < 2 || FZ_SKEW || FZ_PAIRS || FZ_LDS_SLOTS > 0 || FZ_NFR > 0 || FZ_NFW > 0 || FZ_NMOD > 0 || FZ_NCONST64 > 0 || (FZ_FLAGS & FZ_VF_OUT_F64)
#error "PCM frames: two or four streams per lane of a float32 graph whose delay lines live in registers"
#endif
#if !(FZ_FLAGS & 3u)
#error "PCM frames: one side at least is int16 (float32 on both is the frame kernel)"
#endif

#define FZ_PCM_A(n) ((n) > 0 ? (n) : 1)
#define FZ_PCM_NI (FZ_P * FZ_NIN)                /* samples of a lane's slice of an input row */
#define FZ_PCM_NO (FZ_P * FZ_NOUT)               /* ... of an output row */
#define FZ_PCM_IE (FZ_PCM_IN ? 2u : 4u)          /* bytes per sample */
#define FZ_PCM_OE (FZ_PCM_OUT ? 2u : 4u)
// registers a lane's slice of a row travels in: floats as they are, int16 two to a dword -- or, off the grid, one to a register
#define FZ_PCM_RI ((FZ_PCM_IN && !FZ_PCM_B16) ? FZ_PCM_NI / 2 : FZ_PCM_NI)
#define FZ_PCM_RO ((FZ_PCM_OUT && !FZ_PCM_B16) ? FZ_PCM_NO / 2 : FZ_PCM_NO)
#define FZ_PCM_ST_PIECES ((FZ_PCM_OUT && FZ_PCM_B16) ? FZ_PCM_NO : FZ_PCM_A(FZ_PCM_RO) / FZ_VW(FZ_PCM_A(FZ_PCM_RO)))
#define FZ_PCM_AUX_ST (FZ_PCM_ST_PIECES > 1 ? 0 : (FZ_FLAGS & FZ_VF_ST_MERGE) ? 2 : 18)

struct fz_pcm_args {
   const void* in;             // [T][n_streams][n_in]   int16 or float32
   void* out;                  // [T][n_streams][n_out]  int16 or float32
   float* state;               // [n_state][n_streams]
   const float* params;        // [n_param][n_streams]
   unsigned long long n_streams;
   unsigned int n_samples;
   unsigned int n_groups;      // lanes of work: ceil(n_streams / FZ_P)
   float c[FZ_PCM_A(FZ_NCONST)];
};

__device__ __forceinline__ fz_rsrc fz_pcm_rsrc(const void* base, unsigned bytes)
{
   return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, FZ_SRD_FLAGS);
}

__device__ __forceinline__ float fz_pcm_to_float(int q) { return (float)q * 0x1p-15f; }
__device__ __forceinline__ int fz_pcm_from_float(float y)
{
   const float r = y * 32768.0f;
   return r != r ? 0 : r >= 32767.0f ? 32767 : r <= -32768.0f ? -32768 : (int)__builtin_rintf(r);
}

// a lane's slice of an input row into its registers
__device__ __forceinline__ void fz_pcm_load_row(fz_rsrc r, unsigned boff, float (&raw)[FZ_PCM_A(FZ_PCM_RI)])
{
#if FZ_NIN == 0
   (void)r; (void)boff;
   raw[0] = 0.f;
#elif FZ_PCM_IN && FZ_PCM_B16
#pragma unroll
   for (int k = 0; k < FZ_PCM_NI; ++k)
      raw[k] = __builtin_bit_cast(float, (unsigned)__builtin_amdgcn_raw_buffer_load_b16(r, (int)(boff + (unsigned)k * 2u), 0, FZ_AUX_LD));
#else
   fz_load_frame<FZ_PCM_RI>(r, boff, raw);
#endif
}

// sample e of the slice (stream e / FZ_NIN of the lane, wire e % FZ_NIN) as the float the graph reads
__device__ __forceinline__ float fz_pcm_in_sample(const float (&raw)[FZ_PCM_A(FZ_PCM_RI)], int e)
{
#if !FZ_PCM_IN
   return raw[e];
#elif FZ_PCM_B16
   return fz_pcm_to_float((short)__builtin_bit_cast(unsigned, raw[e]));
#else
   return fz_pcm_to_float((short)(__builtin_bit_cast(unsigned, raw[e >> 1]) >> ((e & 1) * 16)));
#endif
}

template <int N, int AUX> __device__ __forceinline__ void fz_pcm_store_dwords(fz_rsrc r, unsigned boff, const unsigned (&d)[N])
{
   constexpr int VW = FZ_VW(N);
#pragma unroll
   for (int k = 0; k < N / VW; ++k) {
      const int o = (int)(boff + (unsigned)(k * VW * 4));
      if constexpr (VW == 4) __builtin_amdgcn_raw_buffer_store_b128((fz_u4){d[4 * k], d[4 * k + 1], d[4 * k + 2], d[4 * k + 3]}, r, o, 0, AUX);
      else if constexpr (VW == 2) __builtin_amdgcn_raw_buffer_store_b64((fz_u2){d[2 * k], d[2 * k + 1]}, r, o, 0, AUX);
      else __builtin_amdgcn_raw_buffer_store_b32(d[k], r, o, 0, AUX);
   }
}

// a lane's slice of an output row: v[e] = sample e (stream e / FZ_NOUT of the lane, wire e % FZ_NOUT)
__device__ __forceinline__ void fz_pcm_store_row(fz_rsrc r, unsigned boff, const float (&v)[FZ_PCM_A(FZ_PCM_NO)])
{
#if FZ_NOUT == 0
   (void)r; (void)boff; (void)v;
#elif !FZ_PCM_OUT
   unsigned d[FZ_PCM_NO];
#pragma unroll
   for (int e = 0; e < FZ_PCM_NO; ++e) d[e] = __builtin_bit_cast(unsigned, v[e]);
   fz_pcm_store_dwords<FZ_PCM_NO, FZ_PCM_AUX_ST>(r, boff, d);
#elif FZ_PCM_B16
#pragma unroll
   for (int e = 0; e < FZ_PCM_NO; ++e)
      __builtin_amdgcn_raw_buffer_store_b16((unsigned short)fz_pcm_from_float(v[e]), r, (int)(boff + (unsigned)e * 2u), 0, FZ_PCM_AUX_ST);
#else
   unsigned d[FZ_PCM_RO];
#pragma unroll
   for (int k = 0; k < FZ_PCM_RO; ++k)
      d[k] = ((unsigned)fz_pcm_from_float(v[2 * k]) & 0xFFFFu) | ((unsigned)fz_pcm_from_float(v[2 * k + 1]) << 16);
   fz_pcm_store_dwords<FZ_PCM_RO, FZ_PCM_AUX_ST>(r, boff, d);
#endif
}

extern "C" __global__ void FZ_BOUNDS FZ_KERNEL(const fz_pcm_args a)
{
   float fz_c[FZ_PCM_A(FZ_NCONST)];
   double fz_cd[1] = {0.0};
#pragma unroll
   for (int k = 0; k < FZ_PCM_A(FZ_NCONST); ++k) fz_c[k] = a.c[k];
   // the block order of the frame kernel: workgroups are dispatched round-robin over the 8 XCDs, each XCD takes one contiguous range of
   // stream groups (blockIdx.x & 7 is the XCD the workgroup sits on)
   unsigned blk = blockIdx.x;
   {
      const unsigned nb = gridDim.x, xcd = blk & 7u, idx = blk >> 3, q = nb >> 3, r = nb & 7u;
      blk = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + idx;
   }
   const unsigned tid = threadIdx.x;
   const unsigned grp = blk * FZ_BLOCK + tid;             // this lane's stream group
   if (grp >= a.n_groups) return;                         // the last block's idle lanes (no barriers below)
   const unsigned soff = grp * FZ_P;                      // first stream of the lane
   const size_t ns = (size_t)a.n_streams;
   const unsigned T = a.n_samples;
   const unsigned ibytes = (unsigned)ns * (FZ_NIN * FZ_PCM_IE), obytes = (unsigned)ns * (FZ_NOUT * FZ_PCM_OE);   // one row (< 4 GiB: the host checks)
   const unsigned ioff = grp * (FZ_PCM_NI * FZ_PCM_IE), ooff = grp * (FZ_PCM_NO * FZ_PCM_OE);                    // the lane's bytes inside a row
   const char* const in0 = static_cast<const char*>(a.in);
   char* op = static_cast<char*>(a.out);                  // the output row at hand (wave-uniform)

   fz_graph G;
   const unsigned ph[1] = {0};
   G.load_params(a.params, ns, soff);
   G.load_state(a.state, ns, soff, (V*)nullptr, tid, ph);

   float xa[FZ_U][FZ_PCM_A(FZ_PCM_RI)], xb[FZ_U][FZ_PCM_A(FZ_PCM_RI)];

// `valid` false: the chunk does not exist.  Its loads are issued all the same, through descriptors of zero bytes (they return 0 and
// touch no memory): conditional loads would make the register buffers loop-carried values the compiler waits for at the loop's end
// (fz_kernel_frames.hip.inc has the measurement).
#define FZ_PCM_LOAD_CHUNK(buf, chunk, valid)                                                                  \
   {                                                                                                          \
      const bool ok_ = (valid);                                                                               \
      const char* const rows_ = in0 + (size_t)(ok_ ? (unsigned)(chunk) : 0u) * FZ_U * ibytes;                 \
      _Pragma("unroll") for (int u = 0; u < FZ_U; ++u)                                                        \
         fz_pcm_load_row(fz_pcm_rsrc(rows_ + (size_t)u * ibytes, ok_ ? ibytes : 0u), ioff, buf[u]);           \
   }

#define FZ_PCM_STEP(raw, tt, orow, uidx)                                                                      \
   {                                                                                                          \
      V x[FZ_PCM_A(FZ_NIN)];                                                                                  \
      VO y[FZ_PCM_A(FZ_NOUT)];                                                                                \
      V hr[1], hw[1];                                                                                         \
      _Pragma("unroll") for (int i = 0; i < FZ_NIN; ++i)                                                      \
         _Pragma("unroll") for (int p = 0; p < FZ_P; ++p) fz_set(x[i], p, fz_pcm_in_sample(raw, p * FZ_NIN + i)); \
      G.step(x, y, fz_c, fz_cd, (V*)nullptr, tid, (tt), hr, hw, (const float*)nullptr, 0u, (uidx));           \
      float fo[FZ_PCM_A(FZ_PCM_NO)];                                                                          \
      _Pragma("unroll") for (int j = 0; j < FZ_NOUT; ++j)                                                     \
         _Pragma("unroll") for (int p = 0; p < FZ_P; ++p) fo[p * FZ_NOUT + j] = fz_get(y[j], p);              \
      fz_pcm_store_row(fz_pcm_rsrc((orow), obytes), ooff, fo);                                                \
   }

#define FZ_PCM_COMPUTE_CHUNK(buf, chunk)                                                                      \
   {                                                                                                          \
      _Pragma("unroll") for (int u = 0; u < FZ_U; ++u)                                                        \
         FZ_PCM_STEP(buf[u], (unsigned)(chunk) * FZ_U + (unsigned)u, op + (size_t)u * obytes, u)              \
      op += (size_t)FZ_U * obytes;                                                                            \
   }

   const unsigned nchunks = T / FZ_U;
   unsigned c = 0;
   FZ_PCM_LOAD_CHUNK(xa, 0, nchunks > 0)
   while (c + 2 <= nchunks) {
      FZ_PCM_LOAD_CHUNK(xb, c + 1, true)
      FZ_PCM_COMPUTE_CHUNK(xa, c)
      FZ_PCM_LOAD_CHUNK(xa, c + 2, c + 2 < nchunks)
      FZ_PCM_COMPUTE_CHUNK(xb, c + 1)
      c += 2;
   }
   if (c < nchunks) {
      FZ_PCM_COMPUTE_CHUNK(xa, c)
      ++c;
   }
   // the rows behind the last whole chunk, one at a time
   for (unsigned t = nchunks * FZ_U; t < T; ++t) {
      float x1[FZ_PCM_A(FZ_PCM_RI)];
      fz_pcm_load_row(fz_pcm_rsrc(in0 + (size_t)t * ibytes, ibytes), ioff, x1);
      FZ_PCM_STEP(x1, t, op, -1)
      op += obytes;
   }

   G.store_state(a.state, ns, soff, (V*)nullptr, tid, T);
}
