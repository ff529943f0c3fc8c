// The state dump of the block-start-states kernels in ring mode (fz_kernel_states.hip.inc, fz_kernel_states_sm.hip.inc with FZ_RING;
// embed.py splices this text in at their `//@splice` line): the whole state in the caller's rows -- the register rows, then every ring
// line read back from its value ring, youngest value first; and with FZ_FAR the far lines' rows of it, fz_dump_far.
static __device__ __forceinline__ void fz_dump_state(float* dst, size_t ns, const float* st, const float* ring, const unsigned* pos)
{
#pragma unroll
   for (int r = 0; r < FZ_NREG; ++r) dst[(size_t)fz_reg_row[r] * ns] = st[r];
#pragma unroll
   for (int l = 0; l < FZ_NRL; ++l) {
      const unsigned D = fz_rl_depth[l];
      unsigned slot = pos[l];                              // (the slot of u[t]: the row before it is u[t-1], the state row row0)
#pragma unroll 4
      for (unsigned j = 0; j < D; ++j) {
         slot = slot ? slot - 1u : D - 1u;
         dst[(size_t)(fz_rl_row0[l] + j) * ns] = ring[(size_t)(fz_rl_slot0[l] + slot) * FZ_BLOCK];
      }
   }
}
#if FZ_FAR
// the far lines' rows of a state dump: every slot of the working ring as it is, the phase row the slot of the row the dump stands before.
// dst and wr are the lane's columns
static __device__ __forceinline__ void fz_dump_far(float* dst, size_t ns, const float* wr, const unsigned* fslot)
{
#pragma unroll
   for (int f = 0; f < FZ_NFL; ++f) {
      const unsigned D = fz_fl_depth[f];
#pragma unroll 4
      for (unsigned k = 0; k < D; ++k) dst[(size_t)(fz_fl_row0[f] + k) * ns] = wr[(size_t)(fz_fl_slot0[f] + k) * ns];
      dst[(size_t)fz_fl_phase_row[f] * ns] = (float)fslot[f];
   }
}
#endif
