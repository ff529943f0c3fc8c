// The patch mover of the stream-major kernels of the adjoint family (fz_kernel_adjoint_sm.hip.inc, fz_kernel_adjoint_ring_sm.hip.inc,
// fz_kernel_states_sm.hip.inc; embed.py splices this text in at their `//@splice` line, behind FZ_AROW, the floats of a padded patch
// row).  The 64 lanes of a wave move a part of a wave-private LDS patch of [64 streams][FZ_AROW] floats as float4 pieces laid along
// the rows: consecutive lanes take consecutive pieces of one stream's run.
#define FZ_AFLIGHT 8                          /* float4 pieces a lane has in flight while a patch part is fetched */

typedef float fz_f4 __attribute__((ext_vector_type(4)));

// orders a wave's own LDS traffic: no workgroup barrier
__device__ __forceinline__ void fz_wave_sync()
{
   __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
   __builtin_amdgcn_wave_barrier();
   __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Piece e = i * 64 + lane of a patch part is piece e % PIECES of patch row e / PIECES: 4 floats at float 4 * (e % PIECES) of that
// stream's run.  `rows` streams of the wave exist, `nval` floats of every run lie inside the window.
// global -> patch: `g` the first float of the wave's first run, `gstride` floats from one stream's run to the next.  No branches (a
// branch per piece of the unrolled loop keeps an exec mask per piece alive in scalar registers): a piece of a missing stream is fetched
// from the wave's last stream, a piece behind the window's last float from the head of its run, and parked where nobody reads it.
template <int PIECES>
__device__ __forceinline__ void fz_patch_fetch(float* part, const float* g, size_t gstride, unsigned rows, unsigned nval, unsigned lane)
{
   constexpr unsigned PP = PIECES > 0 ? PIECES : 1;
#pragma unroll
   for (int i = 0; i < PIECES; ++i) {
      const unsigned e = (unsigned)i * 64u + lane, row = e / PP, q = e % PP;
      const unsigned grow = row < rows ? row : rows - 1u, gq = q * 4u < nval ? q * 4u : 0u;
      *reinterpret_cast<fz_f4*>(part + row * FZ_AROW + q * 4u) = *reinterpret_cast<const fz_f4*>(g + grow * gstride + gq);
      // at most FZ_AFLIGHT pieces in flight: the pieces before are parked before the next are fetched (a wide frame's patch is 20 and
      // more pieces: all of them in registers at once, on top of a chunk's saved states, passed 256 registers)
      if ((i + 1) % FZ_AFLIGHT == 0 && i + 1 < PIECES) asm volatile("" ::: "memory");
   }
}

// patch -> global: the whole pieces inside the window as float4; the floats of the piece that straddles the window's last float (at
// most three) leave one by one, every lane handing over those of its own row
template <int PIECES>
__device__ __forceinline__ void fz_patch_flush(const float* part, float* g, size_t gstride, unsigned rows, unsigned nval, unsigned lane)
{
   constexpr unsigned PP = PIECES > 0 ? PIECES : 1;
#pragma unroll
   for (int i = 0; i < PIECES; ++i) {
      const unsigned e = (unsigned)i * 64u + lane, row = e / PP, q = e % PP;
      if (row < rows && q * 4u + 4u <= nval) *reinterpret_cast<fz_f4*>(g + row * gstride + q * 4u) = *reinterpret_cast<const fz_f4*>(part + row * FZ_AROW + q * 4u);
   }
   const unsigned whole = nval & ~3u;
   if (PIECES > 0 && whole != nval && lane < rows) {
      for (unsigned j = whole; j < nval; ++j) g[lane * gstride + j] = part[lane * FZ_AROW + j];
   }
}
