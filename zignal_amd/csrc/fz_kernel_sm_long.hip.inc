// Part of fz_block_kernel.hip.inc (inlined by embed.py, behind fz_kernel_sm_common.hip.inc): the ONE-STREAM LONG-RUN body for
// stream-major buffers (FZ_VF_SM_LONG, one stream per lane).
// -----------------------------------------------------------------------------------------------------
// LONG-RUN body (1-in/1-out graphs, one stream per lane).  What HBM gives a stream-major walk depends on
// how many contiguous bytes of ONE stream are moved at a time and on where they start (tools/sm_bench.hip,
// profiles/r02/stream_major_access_patterns.txt): 128-byte runs stop at ~5.0 TB/s, 512-byte runs on the 512-byte
// grid reach 6.0-6.3 TB/s; WRITE runs that start off the grid lose 15 % (a whole line off) to 40 % (32 bytes off:
// partial lines), READ runs off the grid about 10 %.  So a phase moves FZ_U = 128 samples (512 B) per stream:
//   * the wave's patch is [64 rows][FZ_U + 12] floats of LDS: inputs of the phase at slots [FZ_LAG, FZ_LAG + FZ_U), the
//     outputs are written IN PLACE behind the read position (slot u + FZ_OSH by the step that consumed slot u + FZ_LAG);
//   * the next run is fetched straight away into FZ_U/4 staging float4 per lane (buffer loads through a per-wave
//     descriptor: rows past the last stream and runs past the last phase are out of its range and read as zero, so
//     the pipeline has no conditional loads) and parked in LDS only when the current phase is done -- a whole phase
//     (~7 us) hides the HBM latency, which one wave per SIMD (the patches of four waves fill the CU's LDS) needs;
//   * the lane reads its own row with ds_read_b128 one group of four samples ahead and writes outputs back as
//     aligned float4 groups; the steps of a phase run in a real loop of 16 unrolled steps (small code);
//   * with stage packing the outputs lag the inputs by FZ_SKEW samples.  The OUTPUT runs stay on the grid (slot k of
//     phase p = output sample p * FZ_U + k); it is the INPUT run of a phase that is taken FZ_LAG = 4, 8 or 12 samples
//     ahead (input samples [p * FZ_U + FZ_LAG, (p + 1) * FZ_U + FZ_LAG)): a prologue of FZ_LAG scalar steps eats the
//     first FZ_LAG inputs, and the last FZ_LAG steps of the last phase run masked on whatever lies behind the block.
// -----------------------------------------------------------------------------------------------------
#if !(FZ_FLAGS & FZ_VF_SM_LONG) || FZ_P != 1 || FZ_NIN != 1 || FZ_NOUT != 1 || FZ_LDS_SLOTS != 0 || (FZ_U % 16) != 0 || FZ_SKEW > 12
#error "long-run stream-major body: 1-in/1-out graph, one stream per lane, no LDS delay rings, unroll % 16 == 0"
#endif
#define FZ_LAG (((FZ_SKEW + 3) / 4) * 4)     /* samples by which the in-run of a phase runs ahead: the skew rounded up to whole float4 */
#define FZ_OSH (FZ_LAG - FZ_SKEW)            /* the output of local step u lands in slot u + FZ_OSH (0..3); its input sat in slot u + FZ_LAG */
#define FZ_LROW (FZ_U + 12)                  /* FZ_LAG head slots + FZ_U, the row stride 4 mod 8 floats: own-row b128 accesses conflict-free */
// With stage packing the in-run of a phase leads the out-run by FZ_LAG samples, i.e. it starts 16-48 bytes off the 128-byte
// line grid: every run then touches FIVE lines for four lines of data, and the line that straddles two phases is fetched by
// both -- 8.6 % more HBM traffic than the algorithm needs (PMC, round 3: 1.0856 x; profiles/r03/rocprofv3_summary.json).
// So the LOADS are line-aligned: load p fetches samples [p U + 32, (p+1) U + 32) of every row, exactly four whole lines.  Its
// last FZ_LCARRY = 32 - FZ_LAG samples belong to the NEXT phase: the lanes that fetched them (piece index >= FZ_LNQ -- the
// piece of a lane is the same in every load) keep them in registers for one more phase, which takes a second staging
// buffer (the lone wave has 512 registers) and no LDS; at staging time those lanes park what they fetched a phase ago, the
// others what they have just fetched.
#define FZ_LSH (FZ_LAG > 0 ? 32 : 0)                  /* samples by which the LOADS lead the out-run grid: one line */
#define FZ_LCARRY (FZ_LSH - FZ_LAG)                   /* 20 / 24 / 28 samples of a load that wait for the next phase */
#define FZ_LNQ ((FZ_U - FZ_LCARRY) / 4)               /* pieces of a load that are parked right away */
#define FZ_LPP (FZ_U / 4)                    /* float4 pieces per stream and phase = pieces per lane and phase */
#define FZ_LFB (FZ_U >= 128 ? 8 : 2)         /* pieces per batch of the out-run (LDS reads first, then the stores); two batches in flight: 64 registers, 16 where two waves share a SIMD */

extern "C" __global__ void FZ_BOUNDS FZ_KERNEL(const fz_args a)
{
   __shared__ float fz_lpatch[FZ_BLOCK / 64][64][FZ_LROW];
   unsigned blk = blockIdx.x;
#ifndef FZ_DBG_NO_XCD_REMAP   /* (kernel experiments: the plain block order) */
   {
      const unsigned nb = gridDim.x, xcd = blk & 7u, idx = blk >> 3, q = nb >> 3, r = nb & 7u;
      blk = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + idx;
   }
#endif
   const unsigned tid = threadIdx.x, lane = tid & 63u;
   // (wave-uniform on purpose: the buffer descriptors below are built from it and must live in SGPRs -- a descriptor the
   // compiler cannot prove uniform costs a 15-instruction waterfall loop around EVERY load and store)
   const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
   const unsigned grp = blk * FZ_BLOCK + tid;
   const size_t ns = (size_t)a.n_streams;
   const size_t s_base = (size_t)blk * FZ_BLOCK + wave * 64u;          // first stream of this wave
   if (s_base >= ns) return;                                         // (no workgroup barriers below)
   const bool active = grp < a.n_groups;
   const unsigned sg = active ? grp : a.n_groups - 1u;                // idle lanes shadow the last stream, store nothing
   const unsigned T = a.n_samples;
   const size_t irow = a.rows_total, orow = a.rows_total;            // floats per stream
   const float* const inw = a.in + a.row0;
   float* const outw = a.out + a.row0;
   float(*patch)[FZ_LROW] = fz_lpatch[wave];
   unsigned ph0[1] = {0};

   fz_graph G;
   G.mod = a.mod + a.row0;
   G.mod_stride = a.mod_stride;
   G.load_params(a.params, ns, sg);
   G.load_state(a.state, ns, sg, FZ_RING, tid, ph0);

   // per-wave buffer descriptors over the WHOLE rows of its (up to) 64 streams (a run that sticks out of the last row is
   // out of range and reads as zero); the piece of lane l in load i sits e = i * 64 + l pieces into the phase: row
   // e / FZ_LPP, piece e % FZ_LPP.  The row goes into the VECTOR offset: that is what the range check looks at.
   const unsigned rows_here = (unsigned)((ns - s_base) < 64u ? (ns - s_base) : 64u);
   const unsigned nph = T / FZ_U;                                     // full phases
   const float* const ibase = a.in + s_base * irow;
   float* const obase = a.out + s_base * orow;
   const unsigned rows_per_load = 64u / FZ_LPP > 0 ? 64u / FZ_LPP : 1u;   // FZ_U = 128: two rows per load instruction
   const unsigned l_row = lane / FZ_LPP, l_q = lane % FZ_LPP;          // (FZ_LPP <= 64: a load covers whole rows)
   const unsigned ivoff = (unsigned)(l_row * irow * 4u + l_q * 16u), ovoff = (unsigned)(l_row * orow * 4u + l_q * 16u);

   fz_f4 stga[FZ_LPP], stgb[FZ_LPP];                                  // two staging buffers in turn (one when the loads need no carry)
   // (phase -1: the load whose tail are the first samples of phase 0; its offset wraps around for the rows it does not reach
   //  -- unsigned arithmetic -- and those pieces are out of the descriptor's range or never looked at)
#define FZ_L_LOAD(buf, phase, valid, voff)                                               \
   {                                                                                     \
      const fz_rsrc ri_ = fz_make_rsrc(ibase, (valid) && fz_dbg_ld ? (unsigned)(rows_here * irow * 4u) : 0u); \
      const unsigned p0_ = (valid) ? (a.row0 + (unsigned)(phase) * FZ_U + (unsigned)(FZ_LSH ? FZ_LSH : FZ_LAG)) * 4u : 0u;   \
      _Pragma("unroll") for (int i = 0; i < FZ_LPP; ++i)                                 \
         buf[i] = fz_buf<4>::ld(ri_, (voff) + p0_ + (unsigned)i * rows_per_load * (unsigned)(irow * 4u)); \
   }
   // park the in-run of a phase: the pieces just fetched (cur) behind the FZ_LCARRY samples that came with the load before (prev)
#define FZ_L_STAGE(cur, prev)                                                            \
   if (FZ_LSH == 0 || l_q < (unsigned)FZ_LNQ) {                                          \
      _Pragma("unroll") for (int i = 0; i < FZ_LPP; ++i)                                 \
         *reinterpret_cast<fz_f4*>(&patch[(unsigned)i * rows_per_load + l_row][(unsigned)(FZ_LAG + FZ_LCARRY) + l_q * 4u]) = cur[i];   \
   } else {                                                                              \
      _Pragma("unroll") for (int i = 0; i < FZ_LPP; ++i)                                 \
         *reinterpret_cast<fz_f4*>(&patch[(unsigned)i * rows_per_load + l_row][(unsigned)FZ_LAG + (l_q - (unsigned)FZ_LNQ) * 4u]) = prev[i];   \
   }
   // out-run of phase `phase`: slot k = output sample phase * FZ_U + k (on the 512-byte grid of the row)
#define FZ_L_FLUSH(phase)                                                                \
   {                                                                                     \
      const fz_rsrc ro_ = fz_make_rsrc(obase, fz_dbg_st ? (unsigned)(rows_here * orow * 4u) : 0u);   \
      const unsigned vo_ = ovoff + (a.row0 + (unsigned)(phase) * FZ_U) * 4u;             \
      /* in batches of FZ_LFB pieces, the LDS reads of a batch ahead of the stores of the batch before.  Left to itself the    \
         compiler reads ONE piece, waits for it, stores it and takes the next one into the same registers: 32 LDS latencies  \
         in a row per phase (15 % of the lone wave's time) */                            \
      fz_f4 va_[FZ_LFB], vb_[FZ_LFB];                                                    \
      _Pragma("unroll") for (int i = 0; i < FZ_LFB; ++i)                                 \
         va_[i] = *reinterpret_cast<const fz_f4*>(&patch[(unsigned)i * rows_per_load + l_row][l_q * 4u]); \
      _Pragma("unroll") for (int b = 0; b < FZ_LPP; b += FZ_LFB)                         \
      {                                                                                  \
         __builtin_amdgcn_sched_barrier(0);                                              \
         if (b + FZ_LFB < FZ_LPP) {                                                      \
            _Pragma("unroll") for (int i = 0; i < FZ_LFB; ++i)                           \
               ((b / FZ_LFB) % 2 ? va_ : vb_)[i] = *reinterpret_cast<const fz_f4*>(&patch[(unsigned)(b + FZ_LFB + i) * rows_per_load + l_row][l_q * 4u]); \
         }                                                                               \
         __builtin_amdgcn_sched_barrier(0);                                              \
         _Pragma("unroll") for (int i = 0; i < FZ_LFB; ++i)                              \
            fz_buf<4>::st(ro_, vo_ + (unsigned)(b + i) * rows_per_load * (unsigned)(orow * 4u), ((b / FZ_LFB) % 2 ? vb_ : va_)[i]); \
      }                                                                                  \
      __builtin_amdgcn_sched_barrier(0);                                                 \
   }

   float c1 = 0.f, c2 = 0.f, c3 = 0.f;                                // the last three outputs (float4 groups straddle steps)
#if FZ_SKEW
   auto seg_mask = [&](unsigned s) {                                  // segment j runs at step s iff j <= s < T + j
      unsigned m = 0;
      for (unsigned j = 0; j < FZ_NSEG; ++j)
         if (j <= s && s - j < T) m |= 1u << j;
      return m;
   };
   // prologue: the first FZ_LAG steps, every lane on its own row; their outputs (samples 0 .. FZ_OSH - 1) go into the carry
   _Pragma("unroll") for (int k = 0; k < FZ_LAG; ++k)
   {
      V x[1];
      VO y[1];
      x[0] = (unsigned)k < T ? inw[(size_t)sg * irow + k] : 0.f;
      G.template step2<true>(x, y, a.c, seg_mask((unsigned)k));
      c3 = c2;
      c2 = c1;
      c1 = y[0];
   }
#define FZ_L_STEP(MASKED, u16)                                                           \
   if (MASKED) G.template step2<true>(x, y, a.c, seg_mask(t0 + (unsigned)FZ_LAG + u0 + (unsigned)(u16)));   \
   else G.template step2<false>(x, y, a.c, 0u);
#else
#define FZ_L_STEP(MASKED, u16)                                                           \
   {                                                                                     \
      V hr[1], hw[1];                                                                    \
      G.step(x, y, a.c, a.cd, FZ_RING, tid, t0 + u0 + (unsigned)(u16), hr, hw, G.mod + (t0 + u0 + (unsigned)(u16)), G.mod_stride);          \
   }
#endif
   // sixteen unrolled steps; MASKED: the closing steps of the block (stage packing), where the input is exhausted
#define FZ_L_BODY16(MASKED)                                                              \
   _Pragma("unroll") for (int k = 0; k < 4; ++k)                                         \
   {                                                                                     \
      const fz_f4 xv = xn;                                                               \
      if (k < 3 || u0 + 16u < (unsigned)FZ_U)      /* one group ahead (not past the end of the phase: the row ends there) */ \
         xn = *reinterpret_cast<const fz_f4*>(&patch[lane][(unsigned)FZ_LAG + u0 + (unsigned)k * 4u + 4u]);   \
      _Pragma("unroll") for (int j = 0; j < 4; ++j)                                      \
      {                                                                                  \
         const int u16 = k * 4 + j;                                                      \
         V x[1];                                                                         \
         VO y[1];                                                                        \
         x[0] = xv[j];                                                                   \
         FZ_L_STEP(MASKED, u16)                                                          \
         if ((u16 + FZ_OSH) % 4 == 3) {                                                  \
            const fz_f4 o_ = {c3, c2, c1, y[0]};                                         \
            *reinterpret_cast<fz_f4*>(&patch[lane][u0 + (unsigned)(u16 + FZ_OSH - 3)]) = o_;   \
         }                                                                               \
         c3 = c2;                                                                        \
         c2 = c1;                                                                        \
         c1 = y[0];                                                                      \
      }                                                                                  \
   }

#if FZ_SKEW
#define FZ_L_COMPUTE(ph)                                                                 \
   {                                                                                     \
      const unsigned u_plain = (ph) + 1u < nph ? (unsigned)FZ_U : (unsigned)FZ_U - 16u;   /* the last 16 steps of the block run masked */ \
      for (; u0 < u_plain; u0 += 16) { FZ_L_BODY16(false) }                              \
      if (u0 < FZ_U) { FZ_L_BODY16(true) }                                               \
   }
#else
#define FZ_L_COMPUTE(ph) for (; u0 < FZ_U; u0 += 16) { FZ_L_BODY16(false) }
#endif
   // one phase: park its in-run (fetched a phase ago into `cur`, its head into `prev` two phases ago), request the next one
   // into the buffer that has just been emptied, compute, hand the out-run back
#define FZ_L_PHASE(ph, cur, prev, nxt)                                                   \
   {                                                                                     \
      const unsigned t0 = (ph) * FZ_U;                                                   \
      (void)t0;                                                                          \
      FZ_SM_CLK(0)                                                                       \
      FZ_SM_CLK_WAITLOADS(32)   /* (the 32 stores of the last out-run are newer) */      \
      FZ_SM_CLK(1)                                                                       \
      FZ_L_STAGE(cur, prev)                                                              \
      fz_wave_sync();                                                                    \
      FZ_SM_CLK(2)                                                                       \
      FZ_L_LOAD(nxt, (ph) + 1u, (ph) + 1u < nph, ivoff)                                  \
      FZ_SM_CLK(3)                                                                       \
      fz_f4 xn = *reinterpret_cast<const fz_f4*>(&patch[lane][FZ_LAG]);                  \
      unsigned u0 = 0;                                                                   \
      FZ_L_COMPUTE(ph)                                                                   \
      fz_wave_sync();                                                                    \
      FZ_SM_CLK(4)                                                                       \
      FZ_L_FLUSH(ph)                                                                     \
      fz_wave_sync();                                                                    \
      FZ_SM_CLK(5)                                                                       \
   }
   // (the six sections of a phase: waiting for its in-run / parking it / requesting the next one / computing / handing the out-run back)
   FZ_SM_CLK_DECL(6)
#if FZ_LAG > 0
   FZ_L_LOAD(stgb, 0xFFFFFFFFu, nph > 0, ivoff)                      // "phase -1": its tail is the head of phase 0 (one extra run per row and launch: 1.6 % of the reads at 4096 samples)
   FZ_L_LOAD(stga, 0u, nph > 0, ivoff)
   for (unsigned ph = 0; ph < nph; ph += 2) {
      FZ_L_PHASE(ph, stga, stgb, stgb)
      if (ph + 1u < nph) FZ_L_PHASE(ph + 1u, stgb, stga, stga)
   }
#else
   (void)stgb;
   FZ_L_LOAD(stga, 0u, nph > 0, ivoff)
   for (unsigned ph = 0; ph < nph; ++ph) FZ_L_PHASE(ph, stga, stga, stga)
#endif

   {  // what is left (n_samples % FZ_U samples): the outputs still in the carry registers, then one step at a time (the
      // last FZ_SKEW of them masked, no input), every lane on its own rows
      const unsigned t_done = nph * FZ_U;                             // output samples stored so far
      if (active) {
         const float cc[3] = {c1, c2, c3};
         _Pragma("unroll") for (int k = 0; k < FZ_OSH; ++k)
            if (t_done + (unsigned)k < T) outw[(size_t)sg * orow + t_done + (unsigned)k] = cc[FZ_OSH - 1 - k];
      }
#if FZ_SKEW
      for (unsigned s = t_done + FZ_LAG; s < T + FZ_SKEW; ++s) {
         V x[1];
         VO y[1];
         x[0] = s < T ? inw[(size_t)sg * irow + s] : 0.f;
         G.template step2<true>(x, y, a.c, seg_mask(s));
         if (active) outw[(size_t)sg * orow + (s - FZ_SKEW)] = y[0];
      }
#else
      for (unsigned t = t_done; t < T; ++t) {
         V x[1], hr[1], hw[1];
         VO y[1];
         x[0] = inw[(size_t)sg * irow + t];
         G.step(x, y, a.c, a.cd, FZ_RING, tid, t, hr, hw, G.mod + (t), G.mod_stride);
         if (active) outw[(size_t)sg * orow + t] = y[0];
      }
#endif
   }
   if (active) G.store_state(a.state, ns, sg, FZ_RING, tid, T);
   FZ_SM_CLK_WRITE(6)
}
