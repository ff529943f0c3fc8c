// What the far modes (FZ_FAR) of fz_kernel_adjoint_ring.hip.inc, fz_kernel_adjoint_ring_sm.hip.inc, fz_kernel_states.hip.inc and
// fz_kernel_states_sm.hip.inc share: the slot arithmetic of a FAR line's ring in HBM and the value of a far read.  Spliced into each
// of them under `#if FZ_FAR` (embed.py), behind FZ_NT and the generated tables fz_fl_* / fz_fr_*.

// the slot `d` rows back from `slot` in a ring of D slots (slot < D, d <= D; d == D: the slot itself)
__device__ __forceinline__ static unsigned fz_far_back(unsigned slot, unsigned d, unsigned D) { return slot >= d ? slot - d : slot + D - d; }
// the slot `j` rows on from `slot` (slot < D, j < D)
__device__ __forceinline__ static unsigned fz_far_on(unsigned slot, unsigned j, unsigned D) { return slot + j >= D ? slot + j - D : slot + j; }

// the value far read q has at row t in the adjoint kernels: tape row t - d, or for t < d the caller's slot (p0 + t - d) mod D.  tape and
// state are the lane's columns; fp0[f] < the depth of far line f
__device__ __forceinline__ static float fz_far_value(const float* tape, const float* state, size_t ns, const unsigned* fp0, int q, size_t t)
{
   const unsigned f = fz_fr_line[q], d = fz_fr_delay[q], D = fz_fl_depth[f];
   if (t >= d) return tape[((t - d) * FZ_NT + FZ_NRL + f) * ns];
   return state[(size_t)(fz_fl_row0[f] + (fp0[f] + (unsigned)t + D - d) % D) * ns];
}
