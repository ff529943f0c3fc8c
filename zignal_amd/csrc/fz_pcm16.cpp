// Blocks whose frames are 16-bit PCM on one side or on both (include/flowz_hip.h: fz_run_block_pcm16): what the PCM kernel supports,
// its static plan, argument checks and the launch.  The kernel text is the common head of fz_block_kernel.hip.inc, the generated body
// of the frame kernels (gen_body) and fz_kernel_pcm16.hip.inc; the code objects go through the kernel cache as a Variant with
// FZ_VF_PCM16.
// The same for stream-major buffers (fz_run_block_pcm16_stream_major): fz_kernel_pcm16_sm.hip.inc behind the same head and body, a
// Variant with FZ_VF_PCM16 | FZ_VF_PCM16_SM whose U carries the rows of a chunk (pcm16_sm_chunk_rows is their one home).
#include <algorithm>

#include "fz_runtime.hpp"

namespace fz {

constexpr uint32_t kPcmBlock = 256;       // lanes per workgroup
constexpr uint32_t kPcmUnroll = 8;        // rows per chunk buffer (halved until nothing spills: settle_variant)
constexpr uint64_t kPcmStoreGrid = 64;    // output rows that start off this grid share sectors between waves (FZ_VF_ST_MERGE)

std::string pcm16_unsupported_reason(const Graph& g)
{
   if (g.typed) return "typed programs (fz_compile_typed) are not supported with PCM frames";
   if (g.n_mod) return "sample-rate modulators (fz_modulator) are not supported with PCM frames";
   for (uint8_t part : g.out_part)
      if (part) return "complex wires are not supported with PCM frames";
   for (const Line& L : g.lines) {
      if (L.far) return "delay lines deeper than 256 samples (rings in HBM) are not supported with PCM frames";
      if (L.in_lds) return "delay lines deeper than 8 samples (rings in LDS) are not supported with PCM frames";
      if (L.part || L.f64) return "complex or double delay lines are not supported with PCM frames";
   }
   if (g.n_lds_slots || g.max_delay > kRegMaxDepth) return "delay lines deeper than 8 samples are not supported with PCM frames";
   if (!g.consts64.empty()) return "float64 nodes (a C++ double literal, fz_literal_f64) are not supported with PCM frames";
   for (const Node& nd : g.nodes) {
      if (nd.f64) return "float64 nodes (a C++ double literal, fz_literal_f64) are not supported with PCM frames";
      if (nd.kind == FZ_IR_MOD) return "sample-rate modulators (fz_modulator) are not supported with PCM frames";
   }
   return "";
}

static void require_supported(const Graph& g)
{
   const std::string why = pcm16_unsupported_reason(g);
   if (!why.empty()) fail(FZ_E_UNSUPPORTED, why);
}

static void check_types(uint32_t in_type, uint32_t out_type)
{
   if (in_type > FZ_FRAMES_I16 || out_type > FZ_FRAMES_I16) fail(FZ_E_INVALID, "unknown frame type: FZ_FRAMES_F32 or FZ_FRAMES_I16");
   if (in_type == FZ_FRAMES_F32 && out_type == FZ_FRAMES_F32)
      fail(FZ_E_INVALID, "float32 frames on both sides: that block is fz_run_block");
}

static uint32_t bytes_of(uint32_t type) { return type == FZ_FRAMES_I16 ? 2u : 4u; }

// In place: every lane reads a row's slice (stream-major: every piece and every row) before it writes the same bytes -- int16 on both
// sides, as many wires out as in, in == out.  Any other overlap of the two buffers' extents is refused.
static void check_in_place_or_apart(const Graph& g, const void* in, uint64_t ibytes, uint32_t in_type, const void* out, uint64_t obytes, uint32_t out_type)
{
   if (!in || !out || !ibytes || !obytes) return;
   const uintptr_t i0 = reinterpret_cast<uintptr_t>(in), o0 = reinterpret_cast<uintptr_t>(out);
   const bool in_place = i0 == o0 && in_type == FZ_FRAMES_I16 && out_type == FZ_FRAMES_I16 && g.n_in == g.n_out;
   if (!in_place && i0 < o0 + obytes && o0 < i0 + ibytes)
      fail(FZ_E_INVALID, "in and out overlap: in place only with int16 frames on both sides, as many output wires as input wires and in == out");
}

// The plan: ONE choice per (graph width, int16 rows on / off the dword grid).
//   up to two wires a side, on the grid    four streams per lane: a wire's int16 slice is a b64 access, its floats a b128
//   wider frames                           two streams per lane: a slice of eight samples and more per row fills the chunk buffers
//   off the grid (streams x wires odd on an int16 side)   two streams per lane, 2-byte accesses on the int16 sides
// 256 lanes per workgroup, chunks of 8 rows; free-running waves.
static Variant pcm16_plan(const Graph& g, uint32_t in_type, uint32_t out_type, uint64_t n_streams)
{
   const bool i16_in = in_type == FZ_FRAMES_I16, i16_out = out_type == FZ_FRAMES_I16;
   const bool off_grid = (i16_in && ((n_streams * g.n_in) & 1u)) || (i16_out && ((n_streams * g.n_out) & 1u));
   Variant v;
   v.P = (std::max(g.n_in, g.n_out) > 2 || off_grid) ? 2 : 4;
   v.U = kPcmUnroll;
   v.block = kPcmBlock;
   v.flags = FZ_VF_PCM16 | (i16_in ? FZ_VF_PCM16_IN : 0u) | (i16_out ? FZ_VF_PCM16_OUT : 0u) | (off_grid ? FZ_VF_PCM16_B16 : 0u);
   if ((n_streams * g.n_out * bytes_of(out_type)) % kPcmStoreGrid || n_streams % v.P) v.flags |= FZ_VF_ST_MERGE;
   return v;
}

// could pcm16_plan (and the halving of the unroll behind it) have made v for this graph?  (kernel manifests are data from elsewhere)
bool pcm16_variant_fits(const Graph& g, const Variant& v)
{
   constexpr uint32_t sub = FZ_VF_PCM16_IN | FZ_VF_PCM16_OUT | FZ_VF_PCM16_B16;
   if (!(v.flags & FZ_VF_PCM16) || (v.flags & ~(FZ_VF_PCM16 | sub | FZ_VF_ST_MERGE)) || !(v.flags & (FZ_VF_PCM16_IN | FZ_VF_PCM16_OUT))) return false;
   if (!pcm16_unsupported_reason(g).empty()) return false;
   if (v.block != kPcmBlock || v.U == 0 || v.U > kPcmUnroll || (v.U & (v.U - 1))) return false;
   const bool two = std::max(g.n_in, g.n_out) > 2 || (v.flags & FZ_VF_PCM16_B16);
   return v.P == (two ? 2u : 4u);
}

// the kernel a block of this shape runs
static Variant pcm16_variant(fz_program* p, uint32_t in_type, uint32_t out_type, uint64_t n_streams)
{
   if (!p) fail(FZ_E_INVALID, "null program");
   require_supported(p->g);
   check_types(in_type, out_type);
   return settle_variant(p, pcm16_plan(p->g, in_type, out_type, n_streams ? n_streams : (1ull << 20)));
}

// kernarg image of `struct fz_pcm_args` (fz_kernel_pcm16.hip.inc) up to the coefficient tail
struct PcmArgsHeader {
   const void* in;
   void* out;
   float* state;
   const float* params;
   unsigned long long n_streams;
   unsigned int n_samples;
   unsigned int n_groups;
};
static_assert(sizeof(PcmArgsHeader) == 4 * 8 + 8 + 2 * 4, "PcmArgsHeader must match the head of the kernel's fz_pcm_args without padding");

int launch_pcm16(fz_program* p, const void* in, void* out, float* state, const float* params, uint64_t n_streams, uint32_t n_samples,
                 uint32_t in_type, uint32_t out_type, void* stream)
{
   if (!p) fail(FZ_E_INVALID, "null program");
   const Graph& g = p->g;
   require_supported(g);
   check_types(in_type, out_type);
   if (!block_has_work(n_streams, n_samples)) return FZ_OK;   // an empty block: nothing to evaluate, state unchanged
   require_pointer(out, g.n_out, "out", "output wires");
   require_pointer(in, g.n_in, "in", "input wires");
   require_pointer(state, g.n_state, "state", "delay lines");
   require_pointer(params, g.n_param, "params", "per-stream coefficients");
   check_aligned16({{in}, {out}, {state}, {params}});
   // a row through one descriptor, and the last lane's byte offset (its four streams may reach past the row) in 32 bits
   const uint64_t irow = n_streams * g.n_in * bytes_of(in_type), orow = n_streams * g.n_out * bytes_of(out_type);
   const uint64_t lane_streams = (n_streams + 3) / 4 * 4;
   if (lane_streams * std::max<uint64_t>((uint64_t)g.n_in * bytes_of(in_type), (uint64_t)g.n_out * bytes_of(out_type)) >= (1ull << 32))
      fail(FZ_E_UNSUPPORTED, "row longer than 4 GiB: shard the streams");
   check_stream_count(n_streams);
   check_in_place_or_apart(g, in, irow * n_samples, in_type, out, orow * n_samples, out_type);
   require_device();
   const Variant v = settle_variant(p, pcm16_plan(g, in_type, out_type, n_streams));
   void* fn = nullptr;
   (void)get_kernel(p, v, &fn);
   const unsigned groups = (unsigned)((n_streams + v.P - 1) / v.P);
   const PcmArgsHeader h{in, out, state, params, (unsigned long long)n_streams, n_samples, groups};
   KernArgs ka(sizeof h, false, g.consts.size());
   ka.set_header(&h);
   copy_coefficients(ka, p);
   launch_kernel(fn, (groups + v.block - 1) / v.block, v.block, stream, ka);
   return FZ_OK;
}

// ---- stream-major buffers --------------------------------------------------------------------------------------------------------
constexpr uint32_t kPcmSmBlock = 64;             // one wave per workgroup: the LDS patch is wave-private and limits occupancy per wave
constexpr uint32_t kPcmSmMaxRows = 64, kPcmSmMinRows = 8;   // rows per chunk (8 int16 samples are one 16-byte piece)
constexpr uint32_t kPcmSmLdsBytes = 160u * 1024u, kPcmSmMinWaves = 4;   // a CU's LDS, and the waves that must fit into it

// bytes of a wave's LDS patch at U rows per chunk: 64 rows of [U x n_in samples][U x n_out samples][16 bytes of padding]
static uint32_t pcm16_sm_patch_bytes(const Graph& g, bool i16_in, bool i16_out, uint32_t U)
{
   return 64u * (U * (g.n_in * (i16_in ? 2u : 4u) + g.n_out * (i16_out ? 2u : 4u)) + 16u);
}

// Rows per chunk, the ONE rule: the shortest power of two at which a stream's run on every int16 side is a whole 128-byte line
// (64 rows for one wire, 32 for two, 16 for four: half-line write runs are what HBM punishes), halved until four waves' patches
// fit a CU's LDS; never below 8 rows.
static uint32_t pcm16_sm_chunk_rows(const Graph& g, bool i16_in, bool i16_out)
{
   uint32_t wires = 0;                                     // the narrowest int16 side
   if (i16_in && g.n_in) wires = g.n_in;
   if (i16_out && g.n_out) wires = wires ? std::min(wires, g.n_out) : g.n_out;
   uint32_t U = kPcmSmMaxRows;
   while (wires && U > kPcmSmMinRows && (U / 2) * wires * 2u >= 128u) U /= 2;
   while (U > kPcmSmMinRows && (uint64_t)pcm16_sm_patch_bytes(g, i16_in, i16_out, U) * kPcmSmMinWaves > kPcmSmLdsBytes) U /= 2;
   return U;
}

static Variant pcm16_sm_plan(const Graph& g, uint32_t in_type, uint32_t out_type)
{
   const bool i16_in = in_type == FZ_FRAMES_I16, i16_out = out_type == FZ_FRAMES_I16;
   Variant v;
   v.P = 1;
   v.U = pcm16_sm_chunk_rows(g, i16_in, i16_out);
   v.block = kPcmSmBlock;
   v.flags = FZ_VF_PCM16 | FZ_VF_PCM16_SM | (i16_in ? FZ_VF_PCM16_IN : 0u) | (i16_out ? FZ_VF_PCM16_OUT : 0u);
   return v;
}

// could pcm16_sm_plan (and the halving of the chunk behind it) have made v for this graph?
bool pcm16_sm_variant_fits(const Graph& g, const Variant& v)
{
   constexpr uint32_t sides = FZ_VF_PCM16_IN | FZ_VF_PCM16_OUT;
   if ((v.flags & ~sides) != (FZ_VF_PCM16 | FZ_VF_PCM16_SM) || !(v.flags & sides)) return false;
   if (!pcm16_unsupported_reason(g).empty()) return false;
   if (v.P != 1 || v.block != kPcmSmBlock || v.U < kPcmSmMinRows || (v.U & (v.U - 1))) return false;
   return v.U <= pcm16_sm_chunk_rows(g, (v.flags & FZ_VF_PCM16_IN) != 0, (v.flags & FZ_VF_PCM16_OUT) != 0);
}

// The variant that runs: the plan with its chunk halved while the kernel spills into scratch memory -- down to kPcmSmMinRows, one
// int16 piece, and no further: a graph that spills even there runs that kernel as it is, spills and all, as the other kernels do
// (settle_variant would go on to chunks the kernel text has no pieces for).
static Variant pcm16_sm_settle(fz_program* p, Variant v)
{
   while (v.U > kPcmSmMinRows && get_kernel(p, v, nullptr)->res.scratch_bytes != 0) v.U /= 2;
   return v;
}

// the kernel a stream-major block of these frame types runs
static Variant pcm16_sm_variant(fz_program* p, uint32_t in_type, uint32_t out_type)
{
   if (!p) fail(FZ_E_INVALID, "null program");
   require_supported(p->g);
   check_types(in_type, out_type);
   return pcm16_sm_settle(p, pcm16_sm_plan(p->g, in_type, out_type));
}

// kernarg image of `struct fz_pcm_sm_args` (fz_kernel_pcm16_sm.hip.inc) up to the coefficient tail
struct PcmSmArgsHeader {
   const void* in;
   void* out;
   float* state;
   const float* params;
   unsigned long long n_streams;
   unsigned int n_samples;
   unsigned int rows_total;
   unsigned int row0;
   unsigned int reserved0;
};
static_assert(sizeof(PcmSmArgsHeader) == 4 * 8 + 8 + 4 * 4, "PcmSmArgsHeader must match the head of the kernel's fz_pcm_sm_args without padding");

int launch_pcm16_sm(fz_program* p, const void* in, void* out, float* state, const float* params, uint64_t n_streams, uint32_t rows_total,
                    uint32_t row0, uint32_t n_samples, uint32_t in_type, uint32_t out_type, void* stream)
{
   if (!p) fail(FZ_E_INVALID, "null program");
   const Graph& g = p->g;
   require_supported(g);
   check_types(in_type, out_type);
   if (!block_has_work(n_streams, n_samples)) return FZ_OK;   // an empty block: nothing to evaluate, nothing touched
   check_window(rows_total, row0, n_samples);
   check_piece_grid("in", g.n_in, rows_total, row0, in_type == FZ_FRAMES_I16);
   check_piece_grid("out", g.n_out, rows_total, row0, out_type == FZ_FRAMES_I16);
   // (this kernel takes a pointer iff its side has wires)
   if (!g.n_in && in) fail(FZ_E_INVALID, "in must be null: the graph has no input wires");
   require_pointer(in, g.n_in, "in", "input wires");
   if (!g.n_out && out) fail(FZ_E_INVALID, "out must be null: the graph has no output wires");
   require_pointer(out, g.n_out, "out", "output wires");
   require_pointer(state, g.n_state, "state", "delay lines");
   require_pointer(params, g.n_param, "params", "per-stream coefficients");
   check_aligned16({{in}, {out}, {state}, {params}});
   check_in_place_or_apart(g, in, n_streams * rows_total * g.n_in * bytes_of(in_type), in_type, out, n_streams * rows_total * g.n_out * bytes_of(out_type), out_type);
   check_stream_count(n_streams);
   require_device();
   const Variant v = pcm16_sm_settle(p, pcm16_sm_plan(g, in_type, out_type));
   void* fn = nullptr;
   (void)get_kernel(p, v, &fn);
   const PcmSmArgsHeader h{in, out, state, params, (unsigned long long)n_streams, n_samples, rows_total, row0, 0u};
   KernArgs ka(sizeof h, false, g.consts.size());
   ka.set_header(&h);
   copy_coefficients(ka, p);
   launch_kernel(fn, (unsigned)((n_streams + 63u) / 64u), v.block, stream, ka);   // one wave of 64 streams per workgroup
   return FZ_OK;
}

}  // namespace fz

using namespace fz;

extern "C" {

int fz_program_pcm16_check(const fz_program* p)
{
   FZ_GUARD(
      if (!p) fail(FZ_E_INVALID, "null program");
      require_supported(p->g);
      return FZ_OK;)
}

int fz_run_block_pcm16(fz_program* p, const void* in, void* out, float* state, const float* params, uint64_t n_streams, uint32_t n_samples,
                       uint32_t in_type, uint32_t out_type, void* hip_stream)
{
   FZ_GUARD(return launch_pcm16(p, in, out, state, params, n_streams, n_samples, in_type, out_type, hip_stream);)
}

int fz_program_pcm16_resources(fz_program* p, uint32_t in_type, uint32_t out_type, uint64_t n_streams, fz_kernel_resources* out)
{
   FZ_GUARD(
      if (!out) fail(FZ_E_INVALID, "fz_program_pcm16_resources: bad arguments");
      *out = resources_of(p, pcm16_variant(p, in_type, out_type, n_streams));
      return FZ_OK;)
}

long fz_program_pcm16_kernel_symbol(fz_program* p, uint32_t in_type, uint32_t out_type, uint64_t n_streams, char* buf, size_t cap)
{
   return string_result(buf, cap, [&] { const Variant v = pcm16_variant(p, in_type, out_type, n_streams); return kernel_symbol(p->g, v); });
}

long fz_program_pcm16_source(fz_program* p, uint32_t in_type, uint32_t out_type, uint64_t n_streams, char* buf, size_t cap)
{
   return string_result(buf, cap, [&] { const Variant v = pcm16_variant(p, in_type, out_type, n_streams); return full_source(p->g, v); });
}

int fz_run_block_pcm16_stream_major(fz_program* p, const void* in, void* out, float* state, const float* params, uint64_t n_streams,
                                    uint32_t rows_total, uint32_t row0, uint32_t n_samples, uint32_t in_type, uint32_t out_type, void* hip_stream)
{
   FZ_GUARD(return launch_pcm16_sm(p, in, out, state, params, n_streams, rows_total, row0, n_samples, in_type, out_type, hip_stream);)
}

int fz_program_pcm16_stream_major_resources(fz_program* p, uint32_t in_type, uint32_t out_type, fz_kernel_resources* out)
{
   FZ_GUARD(
      if (!out) fail(FZ_E_INVALID, "fz_program_pcm16_stream_major_resources: bad arguments");
      *out = resources_of(p, pcm16_sm_variant(p, in_type, out_type));
      return FZ_OK;)
}

long fz_program_pcm16_stream_major_kernel_symbol(fz_program* p, uint32_t in_type, uint32_t out_type, char* buf, size_t cap)
{
   return string_result(buf, cap, [&] { const Variant v = pcm16_sm_variant(p, in_type, out_type); return kernel_symbol(p->g, v); });
}

long fz_program_pcm16_stream_major_source(fz_program* p, uint32_t in_type, uint32_t out_type, char* buf, size_t cap)
{
   return string_result(buf, cap, [&] { const Variant v = pcm16_sm_variant(p, in_type, out_type); return full_source(p->g, v); });
}

}  // extern "C"
