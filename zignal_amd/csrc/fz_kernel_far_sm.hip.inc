// fz_far_sm_kernel -- hand-written gfx950 (MI355X, CDNA4) forward walk over STREAM-MAJOR float32 buffers for graphs with delay lines
// DEEPER THAN 256 SAMPLES, whose rings live in HBM (include/flowz_hip.h: fz_run_block_far_stream_major).  It follows the common head of
// fz_block_kernel.hip.inc (the types, the generated body) the way fz_kernel_pcm16_sm.hip.inc does, and is a kernel text of its own: no
// other kernel's source holds a line of it.
//
// The arithmetic is the generated fz_graph::step of the frame kernels, unchanged, one stream per lane: the bits of `out` and of every
// state row -- register rows, LDS-ring rows, far-line slots, phase rows -- are fz_run_block's on the transposed frames.
//
// Buffers: in [n_streams][rows_total][n_in], out [n_streams][rows_total][n_out], float32; the block is the window of rows
// [row0, row0 + n_samples).  State, per-stream coefficients and uniform coefficients exactly as for fz_run_block ([row][n_streams]).
//
// Frames (the schedule of fz_kernel_pcm16_sm.hip.inc): the 64 lanes of a wave fetch a chunk [64 streams][FZ_R rows] as 16-byte PIECES
// laid along the rows -- 4 floats; consecutive lanes take consecutive pieces of one stream's run --, park them in the wave's own LDS
// patch, and every lane walks its own patch row in a real loop of groups of FZ_U unrolled steps.  Outputs are written into the patch
// row and leave the same way in reverse.  A patch row is [in part: FZ_R x n_in floats][out part: FZ_R x n_out floats][16 bytes of
// padding]; patch bytes per wave: 64 x (4 FZ_R (n_in + n_out) + 16).  The first FZ_FS_HOLD pieces a lane owes to the NEXT chunk are
// requested before the current chunk's steps and held in registers across them; the pieces behind them are fetched once the steps are
// done, FZ_FS_FLIGHT at a time.
//
// Far lines: the rings stay where the forward keeps them, in the state buffer, one coalesced [row][n_streams] row per slot (line l:
// rows fw_row0[l] .. + fw_depth[l]), read and written in place.  The phase p0 of a line comes from its phase row by one readfirstlane,
// reduced modulo the depth D; row t of the block appends its value (hw) to slot (p0 + t) mod D and reads delay n (hr) from slot
// (p0 + t - n) mod D.  Every slot index is reduced modulo D, so every address is inside the line's rows.
//   * Inside whole chunks a far read comes from a register buffer that was requested ONE GROUP of FZ_U rows AHEAD (fa: the group at
//     hand, fb: the next one; 2 FZ_U FZ_NFR registers).  The request goes by row number, so it crosses patch boundaries.  It is safe
//     because 2 FZ_U <= far_min_read (fz_far_sm.cpp: far_sm_group_rows): the reads of group k are requested before the steps of group
//     k - 1 run; row t >= k FZ_U reads what row t - n wrote, and t - n <= (k + 1) FZ_U - 1 - 2 FZ_U < (k - 1) FZ_U: that row ran
//     before the request was issued.  The slot is overwritten by row t - n + D >= t, behind the read in the lane's own program order.
//     A request past the block's end is in bounds by the modulus, and its value is unused.
//   * The rows behind the last whole chunk read their far values with a load of their own in front of the row: the slot a lane reads
//     is one it stored itself (or the caller's), same-lane program order.
//   * At the end the phase row gets (p0 + T) mod D as a float, as fz_kernel_frames.hip.inc writes it.
//
// LDS rings in the same graph (lines of 9 .. 256 samples) live in LDS as in the short stream-major body: ring[slot][lane of the
// workgroup], FZ_LDS_SLOTS x FZ_BLOCK floats, read in place.  Rings and patches share the workgroup's LDS:
// 4 FZ_LDS_SLOTS FZ_BLOCK + (FZ_BLOCK / 64) x 64 x (4 FZ_R (n_in + n_out) + 16) bytes (fz_far_sm.cpp: far_sm_geometry chooses FZ_BLOCK
// and FZ_R together).
//
// Edges, without a workgroup barrier and without an atomic (fz_fs_wave_sync orders the wave's own patch traffic; a lane's ring column
// and its column of the state buffer are its own):
//   * a wave past the last stream returns whole;
//   * the last wave's missing streams: their lanes shadow the wave's last stream (its run, its patch row, its state, params and far
//     columns) but own the LDS ring column of their threadIdx.x; they store nothing -- no frames, no slots, no state -- and every
//     address they form is in bounds; pieces of missing streams are fetched from the wave's last stream and never stored;
//   * only whole chunks travel as pieces, so no piece reaches outside the window; the rows behind the last whole chunk run one step
//     at a time, every lane on its own run: rows outside the window are never touched.
#define FZ_VF_FAR_SM 262145u
#if FZ_P != 1 || (FZ_BLOCK % 64) != 0 || (FZ_R % FZ_U) != 0 || (FZ_U != 4 && FZ_U != 8 && FZ_U != 16) || FZ_SKEW || FZ_RING_G > 0 || FZ_NMOD > 0 || FZ_FLAGS != FZ_VF_FAR_SM
#error "stream-major far lines: one stream per lane, whole waves, chunks of whole groups of 4, 8 or 16 rows, LDS rings read in place, no modulators"
#endif
#if FZ_NFW == 0 || FZ_NFR == 0
#error "stream-major far lines: a graph without a delay line deeper than 256 samples runs the stream-major kernel"
#endif

#define FZ_FS_A(n) ((n) > 0 ? (n) : 1)
#define FZ_FS_IB (FZ_R * FZ_NIN * 4)                      /* bytes of one stream's in-run of a chunk: the in part of a patch row */
#define FZ_FS_OB (FZ_R * FZ_NOUT * 4)                     /* ... of its out-run: the out part, behind it */
#define FZ_FS_ROW (FZ_FS_IB + FZ_FS_OB + 16)              /* padded patch row */
#define FZ_FS_PI (FZ_FS_IB / 16)                          /* pieces per stream and chunk = pieces per lane and chunk */
#define FZ_FS_PO (FZ_FS_OB / 16)
#define FZ_FS_GI (FZ_U * FZ_NIN)                          /* floats of a group's frames: whole pieces (FZ_U is a multiple of 4) */
#define FZ_FS_GO (FZ_U * FZ_NOUT)
#define FZ_FS_HOLD (FZ_FS_PI < 8 ? FZ_FS_PI : 8)          /* pieces of the next chunk held in registers across a chunk's steps */
#define FZ_FS_FLIGHT 8                                    /* pieces in flight at once behind them */

struct fz_far_sm_args {
   const float* in;            // [n_streams][rows_total][n_in]
   float* out;                 // [n_streams][rows_total][n_out]
   float* state;               // [n_state][n_streams]
   const float* params;        // [n_param][n_streams]
   unsigned long long n_streams;
   unsigned int n_samples;
   unsigned int rows_total;
   unsigned int row0;
   unsigned int reserved0;
   float c[FZ_FS_A(FZ_NCONST)];
   double cd[FZ_FS_A(FZ_NCONST64)];
};

__device__ __forceinline__ void fz_fs_wave_sync()
{
   __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
   __builtin_amdgcn_wave_barrier();
   __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Piece e = i * 64 + lane of a chunk's part is piece e % PIECES of patch row e / PIECES: 16 bytes at byte 16 * (e % PIECES) of that
// stream's run.  `rows` streams of the wave exist.  global -> registers: pieces [FIRST, FIRST + N) of the lane; `g` the first byte of
// the wave's first run, `gstride` bytes from one stream's run to the next.
template <int PIECES, int FIRST, int N>
__device__ __forceinline__ void fz_fs_request(fz_u4 (&h)[FZ_FS_A(N)], const char* g, size_t gstride, unsigned rows, unsigned lane)
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
__device__ __forceinline__ void fz_fs_park(unsigned char* patch, const fz_u4 (&h)[FZ_FS_A(N)], unsigned lane)
{
   constexpr unsigned PP = PIECES > 0 ? PIECES : 1;
#pragma unroll
   for (int i = 0; i < N; ++i) {
      const unsigned e = (unsigned)(FIRST + i) * 64u + lane, row = e / PP, q = e % PP;
      *reinterpret_cast<fz_u4*>(patch + row * FZ_FS_ROW + q * 16u) = h[i];
   }
}
// pieces [FIRST, PIECES) of a chunk's in-run into the patch, FZ_FS_FLIGHT at a time
template <int PIECES, int FIRST>
__device__ __forceinline__ void fz_fs_fetch(unsigned char* patch, const char* g, size_t gstride, unsigned rows, unsigned lane)
{
   if constexpr (FIRST < PIECES) {
      constexpr int N = PIECES - FIRST < FZ_FS_FLIGHT ? PIECES - FIRST : FZ_FS_FLIGHT;
      fz_u4 h[N];
      fz_fs_request<PIECES, FIRST, N>(h, g, gstride, rows, lane);
      fz_fs_park<PIECES, FIRST, N>(patch, h, lane);
      asm volatile("" ::: "memory");                        // (parked before the next are requested)
      fz_fs_fetch<PIECES, FIRST + N>(patch, g, gstride, rows, lane);
   }
}
// the out part of the patch -> global: whole pieces of the streams that exist
template <int PIECES>
__device__ __forceinline__ void fz_fs_flush(const unsigned char* patch, char* g, size_t gstride, unsigned rows, unsigned lane)
{
   constexpr unsigned PP = PIECES > 0 ? PIECES : 1;
#pragma unroll
   for (int i = 0; i < PIECES; ++i) {
      const unsigned e = (unsigned)i * 64u + lane, row = e / PP, q = e % PP;
      if (row < rows)
         __builtin_nontemporal_store(*reinterpret_cast<const fz_u4*>(patch + row * FZ_FS_ROW + FZ_FS_IB + q * 16u),
                                     reinterpret_cast<fz_u4*>(g + row * gstride + q * 16u));
   }
}

extern "C" __global__ void __launch_bounds__(FZ_BLOCK) FZ_KERNEL(const fz_far_sm_args a)
{
   FZ_RING_DECL
   __shared__ __attribute__((aligned(16))) unsigned char fz_fs_patches[FZ_BLOCK / 64][64 * FZ_FS_ROW];
   float fz_c[FZ_FS_A(FZ_NCONST)];
   double fz_cd[FZ_FS_A(FZ_NCONST64)];
#pragma unroll
   for (int k = 0; k < FZ_FS_A(FZ_NCONST); ++k) fz_c[k] = a.c[k];
#pragma unroll
   for (int k = 0; k < FZ_FS_A(FZ_NCONST64); ++k) fz_cd[k] = a.cd[k];
   // the block order of the frame kernels: workgroups are dispatched round-robin over the 8 XCDs, each XCD takes one contiguous range
   // of workgroups (blockIdx.x & 7 is the XCD the workgroup sits on)
   unsigned blk = blockIdx.x;
   {
      const unsigned nb = gridDim.x, xcd = blk & 7u, idx = blk >> 3, q = nb >> 3, r = nb & 7u;
      blk = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + idx;
   }
   const size_t ns = (size_t)a.n_streams;
   const unsigned tid = threadIdx.x, lane = tid & 63u;
   const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(tid >> 6));   // (wave-uniform: addresses built from it stay scalar)
   const size_t s_base = (size_t)blk * FZ_BLOCK + wave * 64u;   // first stream of this wave
   if (s_base >= ns) return;                                 // a wave past the last stream (no workgroup barriers below)
   const unsigned rows_here = (unsigned)(ns - s_base < 64u ? ns - s_base : 64u);
   const bool active = lane < rows_here;
   const unsigned prow = active ? lane : rows_here - 1u;     // idle lanes shadow the wave's last stream, store nothing
   const unsigned s = (unsigned)s_base + prow;               // (< 2^30: the host checks)
   const unsigned T = a.n_samples;
   unsigned char* const patch = fz_fs_patches[wave];
   unsigned char* const mine = patch + prow * FZ_FS_ROW;
   // the wave's first run of each buffer: stream s_base, row row0; and this lane's own runs
   const size_t istride = (size_t)a.rows_total * (FZ_NIN * 4), ostride = (size_t)a.rows_total * (FZ_NOUT * 4);
   const char* const gin = reinterpret_cast<const char*>(a.in) + s_base * istride + (size_t)a.row0 * (FZ_NIN * 4);
   char* const gout = reinterpret_cast<char*>(a.out) + s_base * ostride + (size_t)a.row0 * (FZ_NOUT * 4);

   // the far rings: ph[l] the phase at block start, wpos[l] the slot the current row appends to -- (ph + t) mod D, wave-uniform
   unsigned ph[FZ_NFW], wpos[FZ_NFW];
#pragma unroll
   for (int l = 0; l < FZ_NFW; ++l) {
      ph[l] = __builtin_amdgcn_readfirstlane((unsigned)a.state[(size_t)fz_graph::fw_phase_row[l] * ns + s]) % fz_graph::fw_depth[l];
      wpos[l] = ph[l];
   }

   fz_graph G;
   G.load_params(a.params, ns, s);
   G.load_state(a.state, ns, s, FZ_RING, tid, ph);

   // one step: the far reads of the row in hrp[], its values appended to the far rings behind it
#define FZ_FS_STEP(xs, ys, tt, hrp)                                                                          \
   {                                                                                                         \
      V hw[FZ_NFW];                                                                                          \
      G.step(xs, ys, fz_c, fz_cd, FZ_RING, tid, (tt), hrp, hw, (const float*)nullptr, 0u, -1);               \
      _Pragma("unroll") for (int l = 0; l < FZ_NFW; ++l)                                                     \
      {                                                                                                      \
         if (active) a.state[(size_t)(fz_graph::fw_row0[l] + wpos[l]) * ns + s] = hw[l];                     \
         wpos[l] = wpos[l] + 1u == fz_graph::fw_depth[l] ? 0u : wpos[l] + 1u;                                \
      }                                                                                                      \
   }
   // the far reads of the FZ_U rows of the next group to request: rp[r] is the slot read r takes for its first row (and for the first
   // row of the group behind it afterwards)
#define FZ_FS_REQUEST(buf)                                                                                   \
   _Pragma("unroll") for (int r = 0; r < FZ_NFR; ++r)                                                        \
   {                                                                                                         \
      const unsigned l_ = fz_graph::fr_line[r], D_ = fz_graph::fw_depth[l_];                                 \
      unsigned p_ = rp[r];                                                                                   \
      _Pragma("unroll") for (int j = 0; j < FZ_U; ++j)                                                       \
      {                                                                                                      \
         buf[j][r] = a.state[(size_t)(fz_graph::fw_row0[l_] + p_) * ns + s];                                 \
         p_ = p_ + 1u == D_ ? 0u : p_ + 1u;                                                                  \
      }                                                                                                      \
      rp[r] = p_;                                                                                            \
   }

   const unsigned nchunks = T / FZ_R;
   if (nchunks) {
      unsigned rp[FZ_NFR];
#pragma unroll
      for (int r = 0; r < FZ_NFR; ++r) {                     // (1 <= n <= D: the slot of row 0's read)
         const unsigned l = fz_graph::fr_line[r], D = fz_graph::fw_depth[l], n = fz_graph::fr_n[r];
         rp[r] = ph[l] >= n ? ph[l] - n : ph[l] + D - n;
      }
      V fa[FZ_U][FZ_NFR], fb[FZ_U][FZ_NFR];                  // the far reads of the group at hand, of the next group
      FZ_FS_REQUEST(fa)
      fz_fs_fetch<FZ_FS_PI, 0>(patch, gin, istride, rows_here, lane);
      for (unsigned c = 0; c < nchunks; ++c) {
         const bool more = c + 1u < nchunks;                 // (wave-uniform)
         const char* const gnext = gin + (size_t)(c + 1u) * FZ_FS_IB;
         fz_u4 hold[FZ_FS_A(FZ_FS_HOLD)];
         if (more) fz_fs_request<FZ_FS_PI, 0, FZ_FS_HOLD>(hold, gnext, istride, rows_here, lane);
         fz_fs_wave_sync();                                  // the chunk's in-run is parked; the out-run before it has left
#pragma unroll 1
         for (unsigned u0 = 0; u0 < FZ_R; u0 += FZ_U) {
            FZ_FS_REQUEST(fb)                                // the group behind this one, in this chunk, the next or the tail
            float xi[FZ_FS_A(FZ_FS_GI)], yo[FZ_FS_A(FZ_FS_GO)];
            xi[0] = 0.f;
            yo[0] = 0.f;
#pragma unroll
            for (int k = 0; k < FZ_FS_GI / 4; ++k) {
               const fz_f4 q = *reinterpret_cast<const fz_f4*>(mine + u0 * (FZ_NIN * 4) + k * 16);
               xi[4 * k] = q[0];
               xi[4 * k + 1] = q[1];
               xi[4 * k + 2] = q[2];
               xi[4 * k + 3] = q[3];
            }
#pragma unroll
            for (int j = 0; j < FZ_U; ++j) {
               V x[FZ_FS_A(FZ_NIN)];
               VO y[FZ_FS_A(FZ_NOUT)];
               x[0] = 0.f;
#pragma unroll
               for (int w = 0; w < FZ_NIN; ++w) x[w] = xi[j * FZ_NIN + w];
               FZ_FS_STEP(x, y, c * FZ_R + u0 + (unsigned)j, fa[j])
#pragma unroll
               for (int w = 0; w < FZ_NOUT; ++w) yo[j * FZ_NOUT + w] = y[w];
            }
            if (active) {
#pragma unroll
               for (int k = 0; k < FZ_FS_GO / 4; ++k)
                  *reinterpret_cast<fz_f4*>(mine + FZ_FS_IB + u0 * (FZ_NOUT * 4) + k * 16) = (fz_f4){yo[4 * k], yo[4 * k + 1], yo[4 * k + 2], yo[4 * k + 3]};
            }
#pragma unroll
            for (int j = 0; j < FZ_U; ++j) {
#pragma unroll
               for (int r = 0; r < FZ_NFR; ++r) fa[j][r] = fb[j][r];
            }
         }
         fz_fs_wave_sync();                                  // every lane is done with its in part and has written its out part
         fz_fs_flush<FZ_FS_PO>(patch, gout + (size_t)c * FZ_FS_OB, ostride, rows_here, lane);
         if (more) {
            fz_fs_park<FZ_FS_PI, 0, FZ_FS_HOLD>(patch, hold, lane);
            fz_fs_fetch<FZ_FS_PI, FZ_FS_HOLD>(patch, gnext, istride, rows_here, lane);
         }
      }
   }
   // the rows behind the last whole chunk, one at a time, every lane on its own run; a far read is a load in front of its row
   {
      const float* const li = reinterpret_cast<const float*>(gin + (size_t)prow * istride);
      float* const lo = reinterpret_cast<float*>(gout + (size_t)prow * ostride);
      for (unsigned t = nchunks * FZ_R; t < T; ++t) {
         V x[FZ_FS_A(FZ_NIN)];
         VO y[FZ_FS_A(FZ_NOUT)];
         V h1[FZ_NFR];
         x[0] = 0.f;
#pragma unroll
         for (int w = 0; w < FZ_NIN; ++w) x[w] = li[(size_t)t * FZ_NIN + w];
#pragma unroll
         for (int r = 0; r < FZ_NFR; ++r) {
            const unsigned l = fz_graph::fr_line[r], D = fz_graph::fw_depth[l], n = fz_graph::fr_n[r];
            h1[r] = a.state[(size_t)(fz_graph::fw_row0[l] + (wpos[l] >= n ? wpos[l] - n : wpos[l] + D - n)) * ns + s];
         }
         FZ_FS_STEP(x, y, t, h1)
         if (active) {
#pragma unroll
            for (int w = 0; w < FZ_NOUT; ++w) lo[(size_t)t * FZ_NOUT + w] = y[w];
         }
      }
   }

   if (active) {
      G.store_state(a.state, ns, s, FZ_RING, tid, T);
#pragma unroll
      for (int l = 0; l < FZ_NFW; ++l)                       // ring phase after T samples (exact in float: depth < 2^24)
         a.state[(size_t)fz_graph::fw_phase_row[l] * ns + s] = (float)wpos[l];
   }
}
