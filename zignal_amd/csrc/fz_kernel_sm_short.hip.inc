// Part of fz_block_kernel.hip.inc (inlined by embed.py, behind fz_kernel_sm_common.hip.inc): the SHORT-CHUNK body for
// stream-major buffers -- any wire count, one or two streams per lane: chunks of FZ_U samples transposed through the wave's patch
// [64 FZ_P streams][FZ_SM_ROW floats].  Three schedules in one kernel: wide frames in and narrow frames out hold their outputs
// (FZ_SM_HOLD), one-stream 1-in/1-out graphs may be stage-packed (FZ_SKEW), everything else takes the plain chunks.
#if FZ_FLAGS & FZ_VF_SM_LONG
#error "short-chunk stream-major body: not for the long-run variants"
#endif
/* wide frames in, narrow frames out: the outputs of FZ_NIN / FZ_NOUT chunks leave as ONE out-run (see the FZ_SM_HOLD schedule in the kernel) */
#if !defined(FZ_DBG_NO_HOLD) && FZ_SKEW == 0 && FZ_P == 1 && FZ_NIN >= 4 && FZ_NIN % 4 == 0 && FZ_NOUT < FZ_NIN && FZ_NIN % FZ_NOUT == 0 && \
   (FZ_U * FZ_NOUT) % 4 == 0 && FZ_U % 4 == 0 && (FZ_U * FZ_NIN) / 4 <= 32 && 64 % ((FZ_U * FZ_NIN) / 4) == 0   /* (staging + held outputs: 8 registers per piece) */
#define FZ_SM_HOLD 1
#else
#define FZ_SM_HOLD 0
#endif
extern "C" __global__ void FZ_BOUNDS FZ_KERNEL(const fz_args a)
{
   FZ_RING_DECL
   __shared__ fz_f4 fz_sm_patch[FZ_BLOCK / 64][FZ_SM_SW][FZ_SM_ROW / 4];
   unsigned blk = blockIdx.x;
#ifndef FZ_DBG_NO_XCD_REMAP   /* (kernel experiments: the plain block order) */
   {
      const unsigned nb = gridDim.x, xcd = blk & 7u, idx = blk >> 3, q = nb >> 3, r = nb & 7u;
      blk = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + idx;
   }
#endif
   const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
   const unsigned grp = blk * FZ_BLOCK + tid;            // this lane's stream group (FZ_P adjacent streams)
   const bool active = grp < a.n_groups;                 // every lane stays: it carries pieces of other streams
   const unsigned sg = (active ? grp : a.n_groups - 1u) * FZ_P;   // first stream; idle lanes shadow the last group, store nothing
   const size_t ns = (size_t)a.n_streams;
   const unsigned T = a.n_samples;
   const size_t s_base = ((size_t)blk * FZ_BLOCK + wave * 64u) * FZ_P;      // first stream of this wave
   const size_t irow = (size_t)a.rows_total * FZ_NIN, orow = (size_t)a.rows_total * FZ_NOUT;   // floats per stream
   const float* const inw = a.in + (size_t)a.row0 * FZ_NIN;
   float* const outw = a.out + (size_t)a.row0 * FZ_NOUT;
   fz_f4(*patch)[FZ_SM_ROW / 4] = fz_sm_patch[wave];
   unsigned ph[1] = {0};

   fz_graph G;
   G.mod = a.mod + a.row0;
   G.mod_stride = a.mod_stride;
   G.load_params(a.params, ns, sg);
   G.load_state(a.state, ns, sg, FZ_RING, tid, ph);

#if FZ_SM_HOLD
   // -----------------------------------------------------------------------------------------------------
   // WIDE frames in, narrow frames out (FZ_NIN = FZ_SM_R x FZ_NOUT; the 4-wire sum of config 3: 16 bytes in, 4 bytes out per sample).
   // A chunk of FZ_U samples is a 512-byte in-run per stream but only a 128-byte out-run, and it is the WRITE runs HBM is
   // particular about (tools/sm_bench.hip: read 512 / write 256 bytes 5.7 TB/s, read 256 / write 512 6.07).  So the outputs of
   // FZ_SM_R chunks wait in registers (FZ_SM_R x FZ_SM_PO float4 per lane: their own-row groups) and leave together as out-runs as
   // long as the in-runs -- one transposition through the patch per FZ_SM_R chunks, FZ_SM_PI stores of 64 / FZ_SM_PI whole runs each.
   //   * ONE staging buffer: the in-run of chunk c + 1 is requested as soon as chunk c is parked (its registers are free then) and
   //     has the whole compute phase to arrive; per-wave buffer descriptors over the rows of the wave's 64 streams (rows past the
   //     last stream are out of range: they read as zero and their stores are dropped);
   //   * the steps run in a real loop of four unrolled steps; a step reads its frame from the lane's own patch row one step ahead
   //     and the four outputs of a group go back IN PLACE as float4 (output float o of the chunk at float o of the row: behind the
   //     read position, since FZ_NOUT < FZ_NIN).
   // -----------------------------------------------------------------------------------------------------
#define FZ_SM_R (FZ_NIN / FZ_NOUT)
#define FZ_SMH_SPL (64 / FZ_SM_PI)                       /* streams one load / store instruction covers */
   const unsigned wave_u = (unsigned)__builtin_amdgcn_readfirstlane((int)(tid >> 6));   // (wave-uniform: the descriptors live in SGPRs)
   const size_t s_base_u = ((size_t)blk * FZ_BLOCK + wave_u * 64u);
   if (s_base_u >= ns) return;                                        // (no workgroup barriers below)
   const unsigned rows_here = (unsigned)((ns - s_base_u) < 64u ? (ns - s_base_u) : 64u);
   const float* const ibase = a.in + s_base_u * irow;
   float* const obase = a.out + s_base_u * orow;
   const unsigned l_sl = lane / FZ_SM_PI, l_q = lane % FZ_SM_PI;
   const unsigned ivoff = (unsigned)(l_sl * irow * 4u + l_q * 16u), ovoff = (unsigned)(l_sl * orow * 4u + l_q * 16u);
   fz_f4 stg[FZ_SM_PI], held[FZ_SM_R][FZ_SM_PO];
#define FZ_SMH_LOAD(chunk)                                                               \
   {                                                                                     \
      const fz_rsrc ri_ = fz_make_rsrc(ibase, (unsigned)(rows_here * irow * 4u));        \
      const unsigned p0_ = ivoff + (a.row0 * (unsigned)FZ_NIN + (unsigned)(chunk) * (unsigned)FZ_SM_CI) * 4u;   \
      _Pragma("unroll") for (int i = 0; i < FZ_SM_PI; ++i)                               \
         stg[i] = fz_buf<4>::ld(ri_, p0_ + (unsigned)i * FZ_SMH_SPL * (unsigned)(irow * 4u));   \
   }
#define FZ_SMH_CHUNK(chunk, k, more)                                                     \
   {                                                                                     \
      _Pragma("unroll") for (int i = 0; i < FZ_SM_PI; ++i) patch[(unsigned)i * FZ_SMH_SPL + l_sl][l_q] = stg[i];   \
      fz_wave_sync();                                                                    \
      if (more) FZ_SMH_LOAD((chunk) + 1u)                                                \
      fz_f4 xn[FZ_NIN / 4];                                                              \
      _Pragma("unroll") for (int kk = 0; kk < FZ_NIN / 4; ++kk) xn[kk] = patch[lane][kk]; \
      _Pragma("nounroll") for (unsigned u0 = 0; u0 < FZ_U; u0 += 4) {                    \
         float o_[4 * FZ_NOUT];                                                          \
         _Pragma("unroll") for (int j = 0; j < 4; ++j)                                   \
         {                                                                               \
            V x[FZ_NIN];                                                                 \
            VO y[FZ_NOUT];                                                               \
            V hr[1], hw[1];                                                              \
            _Pragma("unroll") for (int i = 0; i < FZ_NIN; ++i) x[i] = xn[i / 4][i % 4];  \
            if (j < 3 || u0 + 4u < (unsigned)FZ_U) {                                     \
               _Pragma("unroll") for (int kk = 0; kk < FZ_NIN / 4; ++kk)                 \
                  xn[kk] = patch[lane][(u0 + (unsigned)j + 1u) * (FZ_NIN / 4) + (unsigned)kk];   \
            }                                                                            \
            const unsigned t_ = (chunk) * FZ_U + u0 + (unsigned)j;                       \
            G.step(x, y, a.c, a.cd, FZ_RING, tid, t_, hr, hw, G.mod + t_, G.mod_stride); \
            _Pragma("unroll") for (int jj = 0; jj < FZ_NOUT; ++jj) o_[j * FZ_NOUT + jj] = y[jj];   \
         }                                                                               \
         _Pragma("unroll") for (int jj = 0; jj < FZ_NOUT; ++jj)                          \
         {                                                                               \
            const fz_f4 v_ = {o_[jj * 4], o_[jj * 4 + 1], o_[jj * 4 + 2], o_[jj * 4 + 3]};   \
            patch[lane][(u0 / 4u) * FZ_NOUT + (unsigned)jj] = v_;                        \
         }                                                                               \
      }                                                                                  \
      _Pragma("unroll") for (int i = 0; i < FZ_SM_PO; ++i) held[k][i] = patch[lane][i];  \
      fz_wave_sync();                                                                    \
   }
   // out-run `run` (FZ_SM_R chunks, the first nk of them valid): own-row groups back into the patch, read along the rows, stored as whole runs
#define FZ_SMH_FLUSH(run, nk)                                                            \
   {                                                                                     \
      _Pragma("unroll") for (int k = 0; k < FZ_SM_R; ++k)                                \
         _Pragma("unroll") for (int i = 0; i < FZ_SM_PO; ++i) patch[lane][k * FZ_SM_PO + i] = held[k][i];   \
      fz_wave_sync();                                                                    \
      const fz_rsrc ro_ = fz_make_rsrc(obase, (unsigned)(rows_here * orow * 4u));        \
      const unsigned vo_ = l_q < (unsigned)(nk) * FZ_SM_PO ? ovoff + (a.row0 * (unsigned)FZ_NOUT + (unsigned)(run) * (unsigned)FZ_SM_CI) * 4u : 0xFFFFFFF0u;   \
      _Pragma("unroll") for (int i = 0; i < FZ_SM_PI; ++i)                               \
      {                                                                                  \
         const fz_f4 v_ = patch[(unsigned)i * FZ_SMH_SPL + l_sl][l_q];                   \
         fz_buf<4>::st(ro_, vo_ == 0xFFFFFFF0u ? vo_ : vo_ + (unsigned)i * FZ_SMH_SPL * (unsigned)(orow * 4u), v_);   \
      }                                                                                  \
      fz_wave_sync();                                                                    \
   }
   const unsigned nchunks = T / FZ_U;
   unsigned c = 0;
   if (nchunks > 0) FZ_SMH_LOAD(0u)
   for (; c + FZ_SM_R <= nchunks; c += FZ_SM_R) {
      _Pragma("unroll") for (int k = 0; k < FZ_SM_R; ++k) FZ_SMH_CHUNK(c + (unsigned)k, k, c + (unsigned)k + 1u < nchunks)
      FZ_SMH_FLUSH(c / FZ_SM_R, FZ_SM_R)
   }
   if (c < nchunks) {                                    // a last, shorter out-run
      const unsigned rem = nchunks - c;
      _Pragma("unroll") for (int k = 0; k < FZ_SM_R - 1; ++k)
         if ((unsigned)k < rem) FZ_SMH_CHUNK(c + (unsigned)k, k, c + (unsigned)k + 1u < nchunks)
      FZ_SMH_FLUSH(c / FZ_SM_R, rem)
   }
#else
   fz_f4 pa[FZ_SM_PI1 * FZ_P], pb[FZ_SM_PI1 * FZ_P];
   const fz_f4 zero4 = {0.f, 0.f, 0.f, 0.f};

#define FZ_SM_LOAD(pbuf, chunk)                                                          \
   _Pragma("unroll") for (int i = 0; i < FZ_SM_PI * FZ_P; ++i)                           \
   {                                                                                     \
      const unsigned e = (unsigned)i * 64u + lane, sl = e / FZ_SM_PI1, q = e - sl * FZ_SM_PI1; \
      const size_t s_ = s_base + sl;                                                     \
      pbuf[i] = s_ < ns ? __builtin_nontemporal_load(reinterpret_cast<const fz_f4*>(inw + s_ * irow + (size_t)(chunk) * FZ_SM_CI) + q) : zero4; \
   }

#if FZ_SKEW
   // Stage-packed schedule on stream-major buffers (one stream per lane, 1-in/1-out graph): segment j runs at time
   // t-j, so step s consumes input sample s and produces output sample s - FZ_SKEW.  The output chunk therefore
   // completes FZ_SKEW steps into the NEXT compute phase: yo[] lives across chunks, the first FZ_SKEW steps of a
   // phase fill the tail of the previous output chunk, which is then transposed through the patch and stored.
   float yo[FZ_SM_CO];
#define FZ_SM_FLUSH(ochunk)                                                              \
   {                                                                                     \
      _Pragma("unroll") for (int k = 0; k < FZ_SM_PO; ++k)                               \
      {                                                                                  \
         fz_f4 v_;                                                                       \
         _Pragma("unroll") for (int j = 0; j < 4; ++j) v_[j] = yo[k * 4 + j];            \
         patch[lane][k] = v_;                                                            \
      }                                                                                  \
      fz_wave_sync();                                                                    \
      _Pragma("unroll") for (int i = 0; i < FZ_SM_PO; ++i)                               \
      {                                                                                  \
         const unsigned e = (unsigned)i * 64u + lane, sl = e / FZ_SM_PO, q = e - sl * FZ_SM_PO; \
         const size_t s_ = s_base + sl;                                                  \
         const fz_f4 v_ = patch[sl][q];                                                  \
         if (s_ < ns) __builtin_nontemporal_store(v_, reinterpret_cast<fz_f4*>(outw + s_ * orow + (size_t)(ochunk) * FZ_SM_CO) + q); \
      }                                                                                  \
      fz_wave_sync();                                                                    \
   }

#define FZ_SM_COMPUTE(pbuf, chunk)                                                       \
   {                                                                                     \
      _Pragma("unroll") for (int i = 0; i < FZ_SM_PI; ++i)                               \
      {                                                                                  \
         const unsigned e = (unsigned)i * 64u + lane, sl = e / FZ_SM_PI1, q = e - sl * FZ_SM_PI1; \
         patch[sl][q] = pbuf[i];                                                         \
      }                                                                                  \
      fz_wave_sync();                                                                    \
      float xin[FZ_SM_CI];                                                               \
      _Pragma("unroll") for (int k = 0; k < FZ_SM_PI; ++k)                               \
      {                                                                                  \
         const fz_f4 v_ = patch[lane][k];                                                \
         _Pragma("unroll") for (int j = 0; j < 4; ++j) xin[k * 4 + j] = v_[j];           \
      }                                                                                  \
      fz_wave_sync();                                                                    \
      _Pragma("unroll") for (int u = 0; u < FZ_U; ++u)                                   \
      {                                                                                  \
         V x[1];                                                                         \
         VO y[1];                                                                        \
         x[0] = xin[u];                                                                  \
         if (u < FZ_SKEW) {                                                              \
            /* block start: segments j > s have not seen a sample yet */                 \
            if ((chunk) == 0u) G.template step2<true>(x, y, a.c, (2u << u) - 1u);        \
            else G.template step2<false>(x, y, a.c, 0u);                                 \
            yo[(FZ_U - FZ_SKEW + u) % FZ_U] = y[0];                                      \
            if (u == FZ_SKEW - 1 && (chunk) != 0u) FZ_SM_FLUSH((chunk) - 1u)             \
         } else {                                                                        \
            G.template step2<false>(x, y, a.c, 0u);                                      \
            yo[(u - FZ_SKEW) % FZ_U] = y[0];                                             \
         }                                                                               \
      }                                                                                  \
   }
#else
// wide frames (a chunk of one stream's inputs is more than 64 floats, and whole float4 pieces per step): see FZ_SM_COMPUTE
#define FZ_SM_WIDE (FZ_SM_CI > 64 && FZ_NIN % 4 == 0)
#define FZ_SM_XIN (FZ_SM_WIDE ? FZ_NIN : (FZ_SM_CI > 0 ? FZ_SM_CI : 1))
#define FZ_SM_COMPUTE(pbuf, chunk)                                                       \
   {                                                                                     \
      _Pragma("unroll") for (int i = 0; i < FZ_SM_PI * FZ_P; ++i)                        \
      {                                                                                  \
         const unsigned e = (unsigned)i * 64u + lane, sl = e / FZ_SM_PI1, q = e - sl * FZ_SM_PI1; \
         patch[sl][q] = pbuf[i];                                                         \
      }                                                                                  \
      fz_wave_sync();                                                                    \
      float xin[FZ_P][FZ_SM_XIN], yo[FZ_P][FZ_SM_CO];                                    \
      if (!FZ_SM_WIDE) {                                                                 \
         _Pragma("unroll") for (int p = 0; p < FZ_P; ++p)                                \
            _Pragma("unroll") for (int k = 0; k < FZ_SM_PI; ++k)                         \
            {                                                                            \
               const fz_f4 v_ = patch[lane * FZ_P + p][k];                               \
               _Pragma("unroll") for (int j = 0; j < 4; ++j) xin[p][(k * 4 + j) % FZ_SM_XIN] = v_[j]; \
            }                                                                            \
      }                                                                                  \
      _Pragma("unroll") for (int u = 0; u < FZ_U; ++u)                                   \
      {                                                                                  \
         V x[FZ_NIN > 0 ? FZ_NIN : 1];                                                   \
         VO y[FZ_NOUT];                                                                  \
         V hr[1], hw[1];                                                                 \
         if (FZ_SM_WIDE && (u * FZ_NIN) % 4 == 0) {                                      \
            /* wide frames: the chunk's inputs stay in the patch (it is not written before the steps are done) and */ \
            /* are read piece by piece: a register copy of the whole chunk would not fit next to both prefetch buffers */ \
            _Pragma("unroll") for (int p = 0; p < FZ_P; ++p)                             \
               _Pragma("unroll") for (int k = 0; k < (FZ_NIN + 3) / 4; ++k)              \
               {                                                                         \
                  const fz_f4 v_ = patch[lane * FZ_P + p][(u * FZ_NIN) / 4 + k];         \
                  _Pragma("unroll") for (int j = 0; j < 4; ++j) xin[p][(k * 4 + j) % FZ_SM_XIN] = v_[j]; \
               }                                                                         \
         }                                                                               \
         _Pragma("unroll") for (int i = 0; i < FZ_NIN; ++i)                              \
            _Pragma("unroll") for (int p = 0; p < FZ_P; ++p) fz_set(x[i], p, xin[p][FZ_SM_WIDE ? ((u * FZ_NIN) % 4 + i) % FZ_SM_XIN : u * FZ_NIN + i]); \
         G.step(x, y, a.c, a.cd, FZ_RING, tid, (chunk) * FZ_U + u, hr, hw, G.mod + ((chunk) * FZ_U + u), G.mod_stride);              \
         _Pragma("unroll") for (int j = 0; j < FZ_NOUT; ++j)                             \
            _Pragma("unroll") for (int p = 0; p < FZ_P; ++p) yo[p][u * FZ_NOUT + j] = fz_get(y[j], p); \
      }                                                                                  \
      fz_wave_sync();                                                                    \
      _Pragma("unroll") for (int p = 0; p < FZ_P; ++p)                                   \
         _Pragma("unroll") for (int k = 0; k < FZ_SM_PO; ++k)                            \
         {                                                                               \
            fz_f4 v_;                                                                    \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) v_[j] = yo[p][k * 4 + j];      \
            patch[lane * FZ_P + p][k] = v_;                                              \
         }                                                                               \
      fz_wave_sync();                                                                    \
      _Pragma("unroll") for (int i = 0; i < FZ_SM_PO * FZ_P; ++i)                        \
      {                                                                                  \
         const unsigned e = (unsigned)i * 64u + lane, sl = e / FZ_SM_PO, q = e - sl * FZ_SM_PO; \
         const size_t s_ = s_base + sl;                                                  \
         const fz_f4 v_ = patch[sl][q];                                                  \
         if (s_ < ns) __builtin_nontemporal_store(v_, reinterpret_cast<fz_f4*>(outw + s_ * orow + (size_t)(chunk) * FZ_SM_CO) + q); \
      }                                                                                  \
      fz_wave_sync();                                                                    \
   }

#endif   // FZ_SKEW

   const unsigned nchunks = T / FZ_U;
   unsigned c = 0;
   if (nchunks > 0) { FZ_SM_LOAD(pa, 0) }
   while (c + 2 <= nchunks) {
      FZ_SM_LOAD(pb, c + 1)
      FZ_SM_COMPUTE(pa, c)
      if (c + 2 < nchunks) { FZ_SM_LOAD(pa, c + 2) }
      FZ_SM_COMPUTE(pb, c + 1)
      c += 2;
   }
   if (c < nchunks) {
      FZ_SM_COMPUTE(pa, c)
      ++c;
   }
#endif   // FZ_SM_HOLD
#if FZ_SKEW
   {  // the last FZ_SKEW outputs of the chunked part come from steps t_done .. t_done + FZ_SKEW - 1 (masked once the
      // input is exhausted), then the ragged tail: one step at a time, every lane on its own rows
      const unsigned t_done = nchunks * FZ_U;
      auto seg_mask = [&](unsigned s) {
         unsigned m = 0;
         for (unsigned j = 0; j < FZ_NSEG; ++j)
            if (j <= s && s - j < T) m |= 1u << j;
         return m;
      };
      _Pragma("unroll") for (int k = 0; k < FZ_SKEW; ++k)
      {
         const unsigned s = t_done + (unsigned)k;
         V x[1];
         VO y[1];
         x[0] = s < T ? inw[(size_t)sg * irow + s] : 0.f;
         G.template step2<true>(x, y, a.c, seg_mask(s));
         yo[FZ_U - FZ_SKEW + k] = y[0];
      }
      if (nchunks > 0) FZ_SM_FLUSH(nchunks - 1u)
      for (unsigned s = t_done + FZ_SKEW; s < T + FZ_SKEW; ++s) {
         V x[1];
         VO y[1];
         x[0] = s < T ? inw[(size_t)sg * irow + s] : 0.f;
         G.template step2<true>(x, y, a.c, seg_mask(s));
         if (active) outw[(size_t)sg * orow + (s - FZ_SKEW)] = y[0];
      }
   }
#else
   // tail: one step at a time, every lane on its own rows
   for (unsigned t = nchunks * FZ_U; t < T; ++t) {
      V x[FZ_NIN > 0 ? FZ_NIN : 1];
      VO y[FZ_NOUT];
      V hr[1], hw[1];
      _Pragma("unroll") for (int i = 0; i < FZ_NIN; ++i)
         _Pragma("unroll") for (int p = 0; p < FZ_P; ++p) fz_set(x[i], p, inw[(size_t)(sg + p) * irow + (size_t)t * FZ_NIN + i]);
      G.step(x, y, a.c, a.cd, FZ_RING, tid, t, hr, hw, G.mod + (t), G.mod_stride);
      if (active) {
         _Pragma("unroll") for (int j = 0; j < FZ_NOUT; ++j)
            _Pragma("unroll") for (int p = 0; p < FZ_P; ++p) outw[(size_t)(sg + p) * orow + (size_t)t * FZ_NOUT + j] = fz_get(y[j], p);
      }
   }
#endif
   if (active) G.store_state(a.state, ns, sg, FZ_RING, tid, T);
}
