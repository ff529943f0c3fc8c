// The forward of a graph with delay lines deeper than 256 samples (rings in HBM) on STREAM-MAJOR float32 buffers
// (include/flowz_hip.h: fz_run_block_far_stream_major): what the kernel supports, its static plan, argument checks and the launch.
// The kernel text is the common head of fz_block_kernel.hip.inc, the generated body of the frame kernels (gen_body) and
// fz_kernel_far_sm.hip.inc; the code objects go through the kernel cache as a Variant {P = patch rows R, U = group rows G, block,
// FZ_VF_FAR_SM}.  fz_run_block_stream_major and a forward fz_variant that names FZ_VF_STREAM_MAJOR keep refusing such graphs
// (fz_plan.cpp: resolve_stream_major); a graph without a far line runs here what it runs there.
#include <algorithm>

#include "fz_inspect.hpp"
#include "fz_runtime.hpp"

namespace fz {

constexpr uint32_t kFarSmLdsBytes = 160u * 1024u;   // per CU and the most one workgroup may declare (gfx950)
constexpr uint32_t kFarSmMinRows = 16;              // the shortest patch: a multiple of every G
// The two far-read buffers of the kernel (the group at hand, the next group) are 2 G n_far_reads registers; G is halved, not below
// 4, while they pass this bound.  64: with the chunk's held pieces (32), a group's frames and the graph's own values none of the
// kernels of the test graphs, of the random graphs with deep delays and of the bench workloads uses scratch (far_comb: 136 registers
// at G = 16, two waves per SIMD by its LDS anyway).
constexpr uint32_t kFarSmReadRegs = 64;

// the stream-major call's own variant: what a graph without a far line runs
static fz_variant plain_stream_major() { return fz_variant{0, 0, 0, FZ_VF_STREAM_MAJOR}; }

// Rows of one unrolled group, the ONE rule: a read requested a group ahead must touch no slot that the group in between writes,
// 2 G <= far_min_read (fz_lower.cpp serves reads of 8 samples and younger from registers: far_min_read >= 9).  G is the largest
// power of two not above min(16, far_min_read / 2) -- 4, 8 or 16 --, halved, not below 4, while 2 G n_far_reads > kFarSmReadRegs.
static uint32_t far_sm_group_rows(const Graph& g)
{
   const uint32_t cap = std::min<uint32_t>(16u, g.far_min_read / 2);
   uint32_t G = 4;
   while (G * 2 <= cap) G *= 2;
   while (G > 4 && 2 * G * g.far_reads.size() > kFarSmReadRegs) G /= 2;
   return G;
}

// LDS bytes of a workgroup of `block` lanes at R rows per patch: ring[slot][lane] of the lines of 9 .. 256 samples, then one patch
// per wave of 64 rows of [R x n_in floats][R x n_out floats][16 bytes of padding]
static uint64_t far_sm_lds_bytes(const Graph& g, uint32_t block, uint32_t R)
{
   return 4ull * g.n_lds_slots * block + (uint64_t)(block / 64) * 64u * (4ull * R * (g.n_in + g.n_out) + 16u);
}

// Lanes per workgroup and rows per patch, chosen TOGETHER, the one rule: R runs from R0 -- the shortest power of two, at least
// kFarSmMinRows, at which one stream's run in the wider frame is a whole 128-byte line (32 rows for one wire) -- down to
// kFarSmMinRows; per R the block over 256, 128, 64 lanes.  The first pair that fits a CU's LDS twice wins, failing that the first
// that fits once (fz_grad.cpp: ring_sm_geometry is the same rule for the backward).  far_comb: 256 lanes, R = 32, 69 632 bytes,
// two workgroups -- eight waves -- per CU: the geometry fz_states_far_sm_kernel runs it with.  block == 0: nothing fits.
struct FarSmGeometry {
   uint32_t block = 0, R = 0;
};
static FarSmGeometry far_sm_geometry(const Graph& g)
{
   const uint32_t wide = std::max<uint32_t>(std::max(g.n_in, g.n_out), 1);
   uint32_t R0 = kFarSmMinRows;
   while (R0 * wide < 32) R0 *= 2;
   for (uint64_t times : {2u, 1u})
      for (uint32_t R = R0; R >= kFarSmMinRows; R /= 2)
         for (uint32_t b : {256u, 128u, 64u})
            if (times * far_sm_lds_bytes(g, b, R) <= kFarSmLdsBytes) return FarSmGeometry{b, R};
   return FarSmGeometry{};
}

std::string far_sm_unsupported_reason(const Graph& g)
{
   if (g.far_lines.empty()) {                                // fz_run_block_stream_major with a null variant: its scope, its words
      try {
         const fz_variant sm = plain_stream_major();
         (void)resolve_variant(g, &sm, 1ull << 20);
      } catch (const Error& er) {
         return er.msg;
      }
      return "";
   }
   if (g.typed) return "typed programs (fz_compile_typed) are not supported with delay lines deeper than 256 samples on stream-major buffers";
   for (uint8_t part : g.out_part)
      if (part) return "complex wires are not supported with delay lines deeper than 256 samples on stream-major buffers";
   if (g.n_mod) return "sample-rate modulators (fz_modulator) are not supported with delay lines deeper than 256 samples on stream-major buffers";
   for (const Node& nd : g.nodes)
      if (nd.kind == FZ_IR_MOD) return "sample-rate modulators (fz_modulator) are not supported with delay lines deeper than 256 samples on stream-major buffers";
   for (const Line& L : g.lines)
      if (L.far && (L.part || L.f64)) return "complex or double delay lines deeper than 256 samples are not supported on stream-major buffers";
   if (g.far_reads.empty() || g.far_min_read <= kRegMaxDepth) return "internal: a delay line deeper than 256 samples without a read from its ring";
   if (!far_sm_geometry(g).block)
      return "stream-major far forward: the rings of the delay lines of 9 .. 256 samples (" + std::to_string(g.n_lds_slots) + " samples) plus a patch of " +
             std::to_string(kFarSmMinRows) + " rows of " + std::to_string(g.n_in + g.n_out) + " wires, " + std::to_string(far_sm_lds_bytes(g, 64, kFarSmMinRows)) +
             " bytes per 64 lanes, do not fit the " + std::to_string(kFarSmLdsBytes) + " bytes of LDS of a workgroup";
   return "";
}

static void require_supported(const Graph& g)
{
   const std::string why = far_sm_unsupported_reason(g);
   if (!why.empty()) fail(FZ_E_UNSUPPORTED, why);
}

// the plan of a graph WITH a far line: static, nothing measured, nothing settled behind it
static Variant far_sm_plan(const Graph& g)
{
   const FarSmGeometry geo = far_sm_geometry(g);
   Variant v;
   v.P = geo.R;
   v.U = far_sm_group_rows(g);
   v.block = geo.block;
   v.flags = FZ_VF_FAR_SM;
   return v;
}

// is v the Variant far_sm_plan makes for this graph?  (kernel manifests are data from elsewhere)
bool far_sm_variant_fits(const Graph& g, const Variant& v)
{
   if (!is_far_sm(v.flags) || g.far_lines.empty() || !far_sm_unsupported_reason(g).empty()) return false;
   const Variant w = far_sm_plan(g);
   return w.P == v.P && w.U == v.U && w.block == v.block;
}

// the kernel the call runs: the far kernel, or for a graph without a far line the stream-major call's default
static Variant far_sm_variant(fz_program* p)
{
   if (!p) fail(FZ_E_INVALID, "null program");
   require_supported(p->g);
   if (!p->g.far_lines.empty()) return far_sm_plan(p->g);
   const fz_variant sm = plain_stream_major();
   return plan_launch(p, &sm, 1ull << 20, 1u << 20, 0, 0, true, false).main;
}

// kernarg image of `struct fz_far_sm_args` (fz_kernel_far_sm.hip.inc) up to the coefficient tails
struct FarSmArgsHeader {
   const float* in;
   float* out;
   float* state;
   const float* params;
   unsigned long long n_streams;
   unsigned int n_samples;
   unsigned int rows_total;
   unsigned int row0;
   unsigned int reserved0;
};
static_assert(sizeof(FarSmArgsHeader) == 4 * 8 + 8 + 4 * 4, "FarSmArgsHeader must match the head of the kernel's fz_far_sm_args without padding");

int launch_far_sm(fz_program* p, const float* in, float* out, float* state, const float* params, uint64_t n_streams, uint32_t rows_total,
                  uint32_t row0, uint32_t n_samples, void* stream)
{
   if (!p) fail(FZ_E_INVALID, "null program");
   if (!rows_total) fail(FZ_E_INVALID, "rows_total must be > 0");
   const Graph& g = p->g;
   if (g.far_lines.empty()) {                                // same kernel, same bits, same refusals as fz_run_block_stream_major
      const fz_variant sm = plain_stream_major();
      return launch(p, in, out, state, params, n_streams, n_samples, &sm, stream, 0, rows_total, row0);
   }
   require_supported(g);
   if (!block_has_work(n_streams, n_samples)) return FZ_OK;   // an empty block: nothing to evaluate, nothing touched
   check_window(rows_total, row0, n_samples);
   check_piece_grid("in", g.n_in, rows_total, row0, false);
   check_piece_grid("out", g.n_out, rows_total, row0, false);
   require_pointer(out, g.n_out, "out", "output wires");
   require_pointer(in, g.n_in, "in", "input wires");
   require_pointer(state, g.n_state, "state", "delay lines");
   require_pointer(params, g.n_param, "params", "per-stream coefficients");
   check_aligned16({{in}, {out}, {state}, {params}});
   check_stream_count(n_streams);
   require_device();
   const Variant v = far_sm_plan(g);
   void* fn = nullptr;
   (void)get_kernel(p, v, &fn);
   const FarSmArgsHeader h{in, out, state, params, (unsigned long long)n_streams, n_samples, rows_total, row0, 0u};
   KernArgs ka(sizeof h, false, g.consts.size(), g.consts64.size());
   ka.set_header(&h);
   copy_coefficients(ka, p);
   launch_kernel(fn, (unsigned)((n_streams + v.block - 1) / v.block), v.block, stream, ka);
   return FZ_OK;
}

}  // namespace fz

using namespace fz;

extern "C" {

int fz_program_far_stream_major_check(const fz_program* p)
{
   FZ_GUARD(
      if (!p) fail(FZ_E_INVALID, "null program");
      require_supported(p->g);
      return FZ_OK;)
}

int fz_run_block_far_stream_major(fz_program* p, const float* in, float* out, float* state, const float* params, uint64_t n_streams,
                                  uint32_t rows_total, uint32_t row0, uint32_t n_samples, void* hip_stream)
{
   FZ_GUARD(return launch_far_sm(p, in, out, state, params, n_streams, rows_total, row0, n_samples, hip_stream);)
}

FZ_INSPECTION(far_stream_major, , "fz_program_far_stream_major_resources", , far_sm_variant(p))

}  // extern "C"
