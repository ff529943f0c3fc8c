// Part of fz_block_kernel.hip.inc (inlined by embed.py, behind fz_kernel_sm_common.hip.inc): the PAIR LONG-RUN body for
// stream-major buffers (FZ_VF_SM_LONG, two streams per lane).  Why runs of 512 bytes on the 512-byte grid, in-runs fetched a phase
// ahead through per-wave descriptors and outputs written in place: see the one-stream body, fz_kernel_sm_long.hip.inc.
// -----------------------------------------------------------------------------------------------------
// PAIR long-run body (two streams per lane, 1-in/1-out graphs, no stage packing): every graph node is ONE packed instruction for
// the lane's two streams -- 28.0 instructions per stream and step in the loop of the 6-biquad cascade against 30.4 with stage packing
// (whose chain crosses from the low to the high half once per step and whose outputs leave through the high half: two moves per
// step, DESIGN 10.1) -- and the lone wave of a SIMD carries 128 streams.  Two patches
// of 512-byte runs per wave would not fit the LDS, so the phase is cut in two HALVES of FZ_U = 64 samples:
//   * the patch of a wave is [64 lanes][2 * FZ_U + 4] floats: a lane's row holds ITS two streams interleaved, [t][stream], so that
//     one ds_read_b128 delivers two steps as two aligned register pairs and one ds_write_b128 takes two steps of outputs -- no
//     moves on the step path; in place, as in the one-stream body;
//   * in-runs are 256 bytes per stream (one half, fetched a half ahead into 32 staging float4 per lane through the per-wave
//     descriptor) and scattered into the rows with stride-2 dword writes; OUT-runs stay 512 bytes on the 512-byte grid: the
//     outputs of the first half wait in 32 float4 per lane (the lone wave has 512 registers) and leave together with the second
//     half's, the two 256-byte pieces of a run by consecutive stores (what HBM gives: reads 256 / writes 512 bytes 6.07 TB/s,
//     profiles/r02/stream_major_access_patterns.txt).
// -----------------------------------------------------------------------------------------------------
#if !(FZ_FLAGS & FZ_VF_SM_LONG) || FZ_P != 2 || FZ_NIN != 1 || FZ_NOUT != 1 || FZ_LDS_SLOTS != 0 || FZ_SKEW != 0 || FZ_U != 64 || (FZ_FLAGS & FZ_VF_OUT_F64)
#error "pair long-run stream-major body: 1-in/1-out graph, two streams per lane, no LDS delay rings, no stage packing, unroll 64"
#endif
#define FZ_QROW (2 * FZ_U + 4)               /* floats per lane row, 4 mod 8: own-row b128 accesses conflict-free */
#define FZ_QPQ (FZ_U / 4)                    /* float4 pieces per stream and half (16) */
#define FZ_QPP (2 * FZ_U / 4)                /* pieces per lane and half (32) */
#define FZ_QRPL (64 / FZ_QPQ)                /* streams per load / store instruction (4) */
#ifndef FZ_QFB
#define FZ_QFB 4                             /* pieces per batch of the out-run (LDS reads of a batch ahead of the stores of the one before) */
#endif

extern "C" __global__ void FZ_BOUNDS FZ_KERNEL(const fz_args a)
{
   __shared__ float fz_qpatch[FZ_BLOCK / 64][64][FZ_QROW];
   unsigned blk = blockIdx.x;
#ifndef FZ_DBG_NO_XCD_REMAP   /* (kernel experiments: the plain block order) */
   {
      const unsigned nb = gridDim.x, xcd = blk & 7u, idx = blk >> 3, q = nb >> 3, r = nb & 7u;
      blk = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + idx;
   }
#endif
   const unsigned tid = threadIdx.x, lane = tid & 63u;
   const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(tid >> 6));   // (wave-uniform: the descriptors live in SGPRs)
   const unsigned grp = blk * FZ_BLOCK + tid;                         // this lane's pair of streams
   const size_t ns = (size_t)a.n_streams;
   const size_t s_base = ((size_t)blk * FZ_BLOCK + wave * 64u) * 2u;   // first stream of this wave
   if (s_base >= ns) return;                                         // (no workgroup barriers below)
   const bool active = grp < a.n_groups;
   const unsigned sg = (active ? grp : a.n_groups - 1u) * 2u;         // idle lanes shadow the last pair, store nothing
   const unsigned T = a.n_samples;
   const size_t irow = a.rows_total, orow = a.rows_total;            // floats per stream
   const float* const inw = a.in + a.row0;
   float* const outw = a.out + a.row0;
   float(*patch)[FZ_QROW] = fz_qpatch[wave];
   unsigned ph0[1] = {0};

   fz_graph G;
   G.mod = a.mod + a.row0;
   G.mod_stride = a.mod_stride;
   G.load_params(a.params, ns, sg);
   G.load_state(a.state, ns, sg, FZ_RING, tid, ph0);

   // per-wave descriptors over the whole rows of its (up to) 128 streams; piece i of a lane: stream 4 i + lane / 16 of the
   // wave, float4 lane % 16 of the half -- i.e. row 2 i + lane / 32 of the patch, stream lane / 16 % 2 of that row's pair
   const unsigned rows_here = (unsigned)((ns - s_base) < 128u ? (ns - s_base) : 128u);
   const unsigned nph = T / (2u * FZ_U);                              // full phases (two halves each)
   const float* const ibase = a.in + s_base * irow;
   float* const obase = a.out + s_base * orow;
   const unsigned l_row = lane / FZ_QPQ, l_q = lane % FZ_QPQ;
   const unsigned ivoff = (unsigned)(l_row * irow * 4u + l_q * 16u), ovoff = (unsigned)(l_row * orow * 4u + l_q * 16u);
   // Where the float4 group g of a row (steps 2 g, 2 g + 1 of the lane's two streams) sits in the row: at group (g >> 1) + 16 (g & 1).
   // A piece of an in- / out-run (four samples of ONE stream: half of groups 2 q and 2 q + 1) then lands in groups q and q + 16, and
   // the sixteen lanes that move the pieces of one stream hit sixteen different bank quads -- laid out in step order they would be
   // eight dwords apart and lanes q and q + 8 would share a bank.
   const unsigned p_row = l_row >> 1, p_col = l_q * 4u + (l_row & 1u);
#define FZ_QPOS(u0_, k_) ((u0_) + 4u * ((unsigned)(k_) >> 1) + 64u * ((unsigned)(k_) & 1u))   /* group u0 / 2 + k of a row, u0 % 16 == 0, k < 8 */

   fz_f4 stg[FZ_QPP], out0[FZ_QPP];
#define FZ_Q_LOAD(half, valid)                                                           \
   {                                                                                     \
      const fz_rsrc ri_ = fz_make_rsrc(ibase, (valid) && fz_dbg_ld ? (unsigned)(rows_here * irow * 4u) : 0u); \
      const unsigned p0_ = (valid) ? (a.row0 + (unsigned)(half) * FZ_U) * 4u : 0u;       \
      _Pragma("unroll") for (int i = 0; i < FZ_QPP; ++i)                                 \
         stg[i] = fz_buf<4>::ld(ri_, ivoff + p0_ + (unsigned)i * FZ_QRPL * (unsigned)(irow * 4u)); \
   }
#define FZ_Q_STAGE                                                                       \
   _Pragma("unroll") for (int i = 0; i < FZ_QPP; ++i)                                    \
   {                                                                                     \
      float* const d_ = &patch[(unsigned)i * 2u + p_row][p_col];                         \
      d_[0] = stg[i][0];                                                                 \
      d_[2] = stg[i][1];                                                                 \
      d_[64] = stg[i][2];                                                                \
      d_[66] = stg[i][3];                                                                \
   }
#define FZ_Q_GATHER(dst, i)                                                              \
   {                                                                                     \
      const float* const s_ = &patch[(unsigned)(i) * 2u + p_row][p_col];                 \
      dst = (fz_f4){s_[0], s_[2], s_[64], s_[66]};                                       \
   }
   // the FZ_U steps of a half: a lane on its own row, two steps per float4 group, the next group read ahead
#define FZ_Q_COMPUTE(half)                                                               \
   {                                                                                     \
      const unsigned t0 = (unsigned)(half) * FZ_U;                                       \
      fz_f4 xn = *reinterpret_cast<const fz_f4*>(&patch[lane][0]);                       \
      for (unsigned u0 = 0; u0 < FZ_U; u0 += 16) {                                       \
         _Pragma("unroll") for (int k = 0; k < 8; ++k)                                   \
         {                                                                               \
            const fz_f4 xv = xn;                                                         \
            if (k < 7 || u0 + 16u < (unsigned)FZ_U)                                      \
               xn = *reinterpret_cast<const fz_f4*>(&patch[lane][k < 7 ? FZ_QPOS(u0, k + 1) : u0 + 16u]);   \
            fz_f4 o_;                                                                    \
            _Pragma("unroll") for (int j = 0; j < 2; ++j)                                \
            {                                                                            \
               V x[1], hr[1], hw[1];                                                     \
               VO y[1];                                                                  \
               x[0] = (V){xv[2 * j], xv[2 * j + 1]};                                     \
               G.step(x, y, a.c, a.cd, FZ_RING, tid, t0 + u0 + (unsigned)(k * 2 + j), hr, hw, G.mod + (t0 + u0 + (unsigned)(k * 2 + j)), G.mod_stride);   \
               o_[2 * j] = y[0][0];                                                      \
               o_[2 * j + 1] = y[0][1];                                                  \
            }                                                                            \
            *reinterpret_cast<fz_f4*>(&patch[lane][FZ_QPOS(u0, k)]) = o_;               \
         }                                                                               \
      }                                                                                  \
   }
   // out-runs of phase `phase`: the first half's pieces from out0, the second half's from the patch, side by side
#define FZ_Q_FLUSH(phase)                                                                \
   {                                                                                     \
      const fz_rsrc ro_ = fz_make_rsrc(obase, fz_dbg_st ? (unsigned)(rows_here * orow * 4u) : 0u);   \
      const unsigned vo_ = ovoff + (a.row0 + (unsigned)(phase) * 2u * FZ_U) * 4u;        \
      fz_f4 va_[FZ_QFB], vb_[FZ_QFB];                                                    \
      _Pragma("unroll") for (int i = 0; i < FZ_QFB; ++i) FZ_Q_GATHER(va_[i], i)          \
      _Pragma("unroll") for (int b = 0; b < FZ_QPP; b += FZ_QFB)                         \
      {                                                                                  \
         __builtin_amdgcn_sched_barrier(0);                                              \
         if (b + FZ_QFB < FZ_QPP) {                                                      \
            _Pragma("unroll") for (int i = 0; i < FZ_QFB; ++i) FZ_Q_GATHER(((b / FZ_QFB) % 2 ? va_ : vb_)[i], b + FZ_QFB + i)   \
         }                                                                               \
         __builtin_amdgcn_sched_barrier(0);                                              \
         _Pragma("unroll") for (int i = 0; i < FZ_QFB; ++i)                              \
         {                                                                               \
            const unsigned o_ = vo_ + (unsigned)(b + i) * FZ_QRPL * (unsigned)(orow * 4u);   \
            fz_buf<4>::st(ro_, o_, out0[b + i]);                                         \
            fz_buf<4>::st(ro_, o_ + (unsigned)FZ_U * 4u, ((b / FZ_QFB) % 2 ? vb_ : va_)[i]);   \
         }                                                                               \
      }                                                                                  \
      __builtin_amdgcn_sched_barrier(0);                                                 \
   }

   // (the seven sections of a phase: waiting for an in-run / parking it / requesting the next / the steps of the halves / keeping the
   //  first half's outputs / the out-run)
   FZ_SM_CLK_DECL(7)
   FZ_Q_LOAD(0u, nph > 0)
   for (unsigned ph = 0; ph < nph; ++ph) {
      // first half: park, request the second, compute, keep the outputs
      FZ_SM_CLK(0)
      FZ_SM_CLK_WAITLOADS(0)
      FZ_SM_CLK(1)
      FZ_Q_STAGE
      fz_wave_sync();
      FZ_SM_CLK(2)
      FZ_Q_LOAD(2u * ph + 1u, true)
      FZ_SM_CLK(3)
      FZ_Q_COMPUTE(2u * ph)
      fz_wave_sync();
      FZ_SM_CLK(4)
      _Pragma("unroll") for (int i = 0; i < FZ_QPP; ++i) FZ_Q_GATHER(out0[i], i)
      fz_wave_sync();
      FZ_SM_CLK(5)
      // second half: park, request the next phase's first, compute, hand both halves back
      FZ_SM_CLK_WAITLOADS(0)
      FZ_SM_CLK(1)
      FZ_Q_STAGE
      fz_wave_sync();
      FZ_SM_CLK(2)
      FZ_Q_LOAD(2u * ph + 2u, ph + 1u < nph)
      FZ_SM_CLK(3)
      FZ_Q_COMPUTE(2u * ph + 1u)
      fz_wave_sync();
      FZ_SM_CLK(4)
      FZ_Q_FLUSH(ph)
      fz_wave_sync();
      FZ_SM_CLK(6)
   }
   // what is left (n_samples % 128 samples): one step at a time, every lane on its own rows
   for (unsigned t = nph * 2u * FZ_U; t < T; ++t) {
      V x[1], hr[1], hw[1];
      VO y[1];
      x[0] = (V){inw[(size_t)sg * irow + t], inw[(size_t)(sg + 1u) * irow + t]};
      G.step(x, y, a.c, a.cd, FZ_RING, tid, t, hr, hw, G.mod + (t), G.mod_stride);
      if (active) {
         outw[(size_t)sg * orow + t] = y[0][0];
         outw[(size_t)(sg + 1u) * orow + t] = y[0][1];
      }
   }
   if (active) G.store_state(a.state, ns, sg, FZ_RING, tid, T);
   FZ_SM_CLK_WRITE(7)
}
