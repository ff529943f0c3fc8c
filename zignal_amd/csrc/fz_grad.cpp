// The backward (include/flowz_hip.h): what the adjoint kernels support, their checkpoint stride, workgroup, patch length and workspace,
// the argument checks and the launch.  One family of kernels, each a Variant with FZ_VF_ADJOINT that goes through the kernel cache
// (fz_codegen.cpp: the family's table, gen_adjoint_config, gen_adjoint_body):
//
//                                                     time-major frames                 stream-major buffers (FZ_VF_ADJOINT_SM)
//   fz_run_block_grad[_stream_major]                  fz_kernel_adjoint.hip.inc         fz_kernel_adjoint_sm.hip.inc
//   fz_run_block_ring_grad[_stream_major]             fz_kernel_adjoint_ring.hip.inc    fz_kernel_adjoint_ring_sm.hip.inc
//     (delay lines in LDS: FZ_VF_ADJOINT_RING)
//   fz_run_block_far_grad[_stream_major]              the same text with FZ_FAR         the same text with FZ_FAR
//     (delay lines in HBM as well: FZ_VF_ADJOINT_RING | FZ_VF_ADJOINT_FAR)
//   fz_run_recording_grad: the block-start states     fz_kernel_states.hip.inc          fz_kernel_states_sm.hip.inc
//     (FZ_VF_STATES)
//   fz_run_recording_ring_grad[_stream_major]:        the same text with FZ_RING        the same text with FZ_RING
//     the same (FZ_VF_STATES | FZ_VF_ADJOINT_RING)
//   fz_run_recording_far_grad[_for]: the same         the same text with FZ_FAR too     the same text with FZ_FAR too
//     (FZ_VF_STATES | FZ_VF_ADJOINT_RING | FZ_VF_ADJOINT_FAR)
//
// Under a squared-error loss (FZ_VF_ADJOINT_LOSS, the ..._loss_grad calls) each of the adjoint kernels forms dL/dy itself, from a
// target: the same text with FZ_LOSS, the same C, workgroup and workspace.  The ring calls share the checks and the launch with the
// others; for a graph without a ring line each IS its plain sibling (same Variant, kernel, symbol, workspace, bits).  The far calls
// stand to the ring calls as those stand to the plain ones: for a graph without a line deeper than 256 samples each IS its ring
// sibling; with one, the far kernel keeps the pending adjoints of such a line in a ring in the workspace.  The backward of a
// recording is two-level checkpointing: one launch of the states kernel, then the block launches above from the last block to the first.
#include <cmath>
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

#include "fz_inspect.hpp"
#include "fz_runtime.hpp"

namespace fz {

constexpr uint32_t kGradBlock = 256;          // lanes (= streams) per workgroup of the adjoint kernel
constexpr uint32_t kGradMaxCheckpoint = 32;   // the chunk is unrolled: every step's state and frame stay in registers

std::string grad_unsupported_reason(const Graph& g, bool rings_in_lds, bool rings_in_hbm)
{
   if (g.typed) return "typed programs (fz_compile_typed) are not supported by the backward";
   if (g.n_mod) return "sample-rate modulators (fz_modulator) are not supported by the backward";
   for (uint8_t part : g.out_part)
      if (part) return "complex wires are not supported by the backward";
   for (const Line& L : g.lines) {
      if (L.far && !(rings_in_lds && rings_in_hbm)) return "delay lines deeper than 256 samples (rings in HBM) are not supported by the backward";
      if (L.in_lds && !rings_in_lds) return "delay lines deeper than 8 samples (rings in LDS) are not supported by the backward";
      if (L.part || L.f64) return "complex or double delay lines are not supported by the backward";
   }
   if (!rings_in_lds && (g.n_lds_slots || g.max_delay > kRegMaxDepth)) return "delay lines deeper than 8 samples are not supported by the backward";
   for (const Node& nd : g.nodes) {
      if (nd.f64) return "float64 nodes (a C++ double literal, fz_literal_f64) are not supported by the backward";
      if (nd.kind == FZ_IR_MOD) return "sample-rate modulators (fz_modulator) are not supported by the backward";
      if (!adjoint_takes(nd.kind)) return "IR node kind " + std::to_string(nd.kind) + " (complex arithmetic) is not supported by the backward";
   }
   return "";
}

// The chunk of sweep 2 keeps C rows of saved floats in registers next to one step's node values and the accumulators: at most 64 saved
// floats, 16 rows at most.  A row saves its state and frame, n_state + n_in floats; in the ring kernels its register state rows, frame and
// ring reads (for a graph without a ring line the two count the same).  Measured: no graph of tests/test_grad_host.py spills; random graphs
// (tests/grad_fuzz_cells.py) do spill SGPRs into VGPR lanes -- one-state graphs at C = 16 as well as 72-state ones at C = 1, with two
// coefficients as with twenty, so counting n_const here removes nothing -- and none uses scratch: correct, slower.
// The far kernel (a graph with a line deeper than 256 samples): the far reads count among the ring reads, and a row of the fast path
// keeps its slots of the adjoint ring as well -- one per far line (rule 2's) and one per far read (rule 3's target): per row
// n_register_state + n_in + n_ring_reads + n_far_reads + (n_far_lines + n_far_reads), whichever path the chunk then takes.
static uint32_t grad_default_checkpoint(const Graph& g, bool ring)
{
   const RingLayout rl = ring ? ring_layout(g) : RingLayout{};
   const uint32_t per_row = std::max<uint32_t>(ring ? rl.n_reg() + g.n_in + rl.n_rr() + 2 * rl.n_fr() + rl.n_fl() : g.n_state + g.n_in, 1);
   uint32_t C = 16;
   while (C > 1 && C * per_row > 64) C /= 2;
   return C;
}

// The stream-major adjoint kernel moves its frames through a wave-private LDS patch of R rows (fz_kernel_adjoint_sm.hip.inc): a patch
// row is R * (n_in + n_out) + 4 floats, a workgroup holds 4 x 64 of them.  R is a power of two >= 4: long enough that the run of ONE
// stream is a whole 128-byte cache line in the WIDER of the two frames, then doubled towards a line in the narrower one while the
// workgroup's patches stay within half a CU's 160 KB of LDS (two workgroups per CU); and at least C -- so a multiple of C (a power of
// two) and of 4.  A 1-in / 1-out graph: R = 32, 17 KB per wave, 68 KB per workgroup.
constexpr uint32_t kLdsBytes = 160u * 1024u;   // per CU and the most one workgroup may declare (gfx950)
static uint32_t sm_patch_bytes(const Graph& g, uint32_t R) { return (R * (g.n_in + g.n_out) + 4u) * 4u * kGradBlock; }
static uint32_t grad_sm_patch_rows(const Graph& g, uint32_t C)
{
   const uint32_t wide = std::max<uint32_t>(std::max(g.n_in, g.n_out), 1), narrow = std::max<uint32_t>(g.n_in && g.n_out ? std::min(g.n_in, g.n_out) : wide, 1);
   uint32_t R = 4;
   while (R * wide < 32) R *= 2;
   while (R * narrow < 32 && sm_patch_bytes(g, 2 * R) <= kLdsBytes / 2) R *= 2;
   return std::max(R, C);
}

// The block-start-states kernel (FZ_VF_STATES): U, the rows of one unrolled group -- two groups of U * n_in frame registers are alive
// (the group the recursion runs and the one requested for the next trip): 8 rows, halved while a group passes 16 floats.
static uint32_t states_unroll(const Graph& g)
{
   uint32_t U = 8;
   while (U > 1 && U * g.n_in > 16) U /= 2;
   return U;
}

// Its stream-major text moves x through a wave-private LDS patch of R rows like sweep 1 of the stream-major adjoint kernel, but the
// patch carries x only: a patch row is R * n_in + 4 floats.  R is a power of two >= 4 long enough that the run of one stream is a
// whole 128-byte cache line (32 rows for one input wire: 9 KB per wave, 36 KB per workgroup); a multiple of U, which is at most 8
// and at most 16 / n_in.
static uint32_t states_sm_patch_bytes(const Graph& g, uint32_t R) { return g.n_in ? (R * g.n_in + 4u) * 4u * kGradBlock : 0u; }
static uint32_t states_sm_patch_rows(const Graph& g)
{
   uint32_t R = 4;
   while (R * g.n_in < 32 && g.n_in) R *= 2;
   return R;
}

// ---- the ring kernels' LDS: value rings (or pending adjoints) alone on time-major frames, rings and patches on stream-major buffers -----
// The LDS floats of one lane: `slots` of rings (the sum of the ring lines' depths) and, on stream-major buffers, its row of a wave's
// patch: R rows of `wires` floats and `pad` of padding.  A workgroup of `block` lanes holds ring[slots][block] and block / 64 patches
// of [64][R wires + pad] floats: 4 block (slots + R wires + pad) bytes.
struct LaneLds {
   uint32_t slots = 0, wires = 0, pad = 0;
   uint64_t bytes(uint32_t block, uint32_t R) const { return 4ull * block * ((uint64_t)slots + (uint64_t)R * wires + pad); }
};

struct RingSmGeometry {
   uint32_t block = 0, R = 0;   // block == 0: nothing fits
};

// The one home of the rule that chooses the workgroup and the patch length together.  R runs over R0, R0 / 2, ... down to Rmin (powers
// of two); per R the block over 256, 128, 64.  The first pair that fits the LDS twice (two workgroups per CU) wins; failing that the
// first that fits once.  The rule prefers a long run per stream (a whole cache line) over lanes per workgroup: static, not measured
// against the alternative.  Time-major frames have no patch: R0 = Rmin = 1, and the rule is the largest block whose rings fit.
static RingSmGeometry ring_sm_geometry(const LaneLds& lane, uint32_t R0, uint32_t Rmin)
{
   for (uint64_t times : {2u, 1u})
      for (uint32_t R = R0; R >= Rmin; R /= 2)
         for (uint32_t b : {256u, 128u, 64u})
            if (times * lane.bytes(b, R) <= kLdsBytes) return RingSmGeometry{b, R};
   return RingSmGeometry{};
}

static uint32_t checkpoint_of(const Graph& g, uint32_t checkpoint_rows, bool ring = false)
{
   if (checkpoint_rows == 0) return grad_default_checkpoint(g, ring);
   if (checkpoint_rows > kGradMaxCheckpoint || (checkpoint_rows & (checkpoint_rows - 1)))
      fail(FZ_E_INVALID, "checkpoint_rows must be 0 (library default) or a power of two <= 32");
   return checkpoint_rows;
}

static void require_supported(const Graph& g, bool rings_in_lds = false, bool rings_in_hbm = false)
{
   const std::string why = grad_unsupported_reason(g, rings_in_lds, rings_in_hbm);
   if (!why.empty()) fail(FZ_E_UNSUPPORTED, why);
}

// The scope of a call, before anything else is asked of it.  ring: the call is of the ring family -- the ring scope and the ring-fit
// refusal in fz_program_ring_grad_check's words, whichever kernel and layout the call goes on to ask for.  far: the call is of the far
// family (fz_run_block_far_*) -- the ring scope plus float lines deeper than 256 samples, which take no LDS.
static void require_scope(const Graph& g, bool ring, bool far = false)
{
   require_supported(g, ring, far);
   if (!ring) return;
   const LaneLds rings{ring_layout(g).slots};
   if (!ring_sm_geometry(rings, 1, 1).block)
      fail(FZ_E_UNSUPPORTED, "the adjoint rings of the delay lines deeper than 8 samples, " + std::to_string(rings.bytes(64, 1)) + " bytes per 64 lanes (" +
                                std::to_string(rings.slots) + " samples), do not fit the " + std::to_string(kLdsBytes) + " bytes of LDS of a workgroup");
}

// the flag set of an adjoint Variant: the one place that refuses a loss on a graph without outputs
static uint32_t adjoint_flags(const Graph& g, uint32_t family_bits, bool loss)
{
   if (loss && g.n_out == 0) fail(FZ_E_INVALID, "the graph has no output wires: a loss has nothing to compare");
   return FZ_VF_ADJOINT | family_bits | (loss ? FZ_VF_ADJOINT_LOSS : 0u);
}

static uint32_t family_bits(bool ring, bool stream_major) { return (ring ? FZ_VF_ADJOINT_RING : 0u) | (stream_major ? FZ_VF_ADJOINT_SM : 0u); }

// The Variant of a block's backward, whichever call asks: {P = 1 (stream-major: the patch rows R -- codegen puts them into FZ_R and the
// symbol), U = C, block}.  ring: the call is of the ring family; for a graph without a ring line its Variant is the plain one itself
// (same kernel, symbol, workspace, bits).  With a ring line the ring kernel's C, and on stream-major buffers R and the block are chosen
// together: R0 = grad_sm_patch_rows(g, C), Rmin = max(4, C) (multiples of 4 and of C); its patch keeps its padding whatever the wires.
// loss: the kernel forms dL/dy itself (FZ_VF_ADJOINT_LOSS next to the family bits); C, block and workspace do not change with it.
// far: the call is of the far family (a ring call as well); for a graph without a line deeper than 256 samples its Variant is the ring
// call's.  With one: FZ_VF_ADJOINT_RING | FZ_VF_ADJOINT_FAR, the far kernel's C (grad_default_checkpoint), and the workgroup the ring
// rule gives the graph's LDS ring lines alone -- the far lines take no LDS --, 256 lanes without any.  On stream-major buffers
// (fz_kernel_adjoint_ring_sm.hip.inc with FZ_FAR) the same rule chooses R and the block together over those LDS ring slots -- none for a graph
// whose deep lines are all far -- and the patch: the ring call's Rmin and its refusal when nothing fits, and R0 =
// max(grad_sm_patch_rows(g, C) / 2, Rmin), HALF the ring call's: one stream's run is half a cache line in the wider frame.  Measured
// (profiles/r19/far_stream_major.txt): the far kernel waits on the tape and the adjoint ring in HBM, a dependent round trip per row
// on the per-row path, and hides that behind waves; with the ring call's R0 (69 632 bytes of patches per 256 lanes, 138 registers:
// two waves per SIMD) a 2000-sample comb at 1 048 576 x 1024 took 1.16 x the time of the transposing route, with half of it (36 864
// bytes, 121 registers: four waves) 0.87 x; the 65 536 x 4096 lines pay 0.05 of the route's time for the shorter runs.
static Variant block_variant(const Graph& g, uint32_t checkpoint_rows, bool ring, bool stream_major, bool loss, bool far = false)
{
   ring = ring || far;
   require_scope(g, ring, far);
   const RingLayout rl = ring ? ring_layout(g) : RingLayout{};
   const uint32_t slots = rl.slots, wires = g.n_in + g.n_out;
   const bool far_lines = rl.n_fl() != 0;
   Variant v;
   v.P = 1;
   v.U = checkpoint_of(g, checkpoint_rows, slots != 0 || far_lines);
   v.block = kGradBlock;
   v.flags = adjoint_flags(g, family_bits(slots != 0 || far_lines, stream_major) | (far_lines ? FZ_VF_ADJOINT_FAR : 0u), loss);
   if (slots || (far_lines && stream_major)) {
      const LaneLds lane{slots, stream_major ? wires : 0u, stream_major ? 4u : 0u};
      const uint32_t Rmin = stream_major ? std::max<uint32_t>(4u, v.U) : 1u;
      // (far lines: R0 is half the ring kernel's, see above)
      const uint32_t R0 = !stream_major ? 1u : far_lines ? std::max(grad_sm_patch_rows(g, v.U) / 2, Rmin) : grad_sm_patch_rows(g, v.U);
      const RingSmGeometry geo = ring_sm_geometry(lane, R0, Rmin);
      if (!geo.block)                                       // (stream-major only: rings alone fit, require_scope has asked)
         fail(FZ_E_UNSUPPORTED, "stream-major ring backward: the rings of the delay lines deeper than 8 samples (" + std::to_string(slots) + " samples) plus a patch of " +
                                   std::to_string(Rmin) + " rows of " + std::to_string(wires) + " wires, " + std::to_string(lane.bytes(64, Rmin)) +
                                   " bytes per 64 lanes, do not fit the " + std::to_string(kLdsBytes) + " bytes of LDS of a workgroup: a smaller checkpoint_rows shortens the patch");
      v.P = geo.R;
      v.block = geo.block;
   } else if (stream_major) {
      v.P = grad_sm_patch_rows(g, v.U);
      if (sm_patch_bytes(g, v.P) > kLdsBytes)
         fail(FZ_E_UNSUPPORTED, "stream-major backward: a patch of " + std::to_string(v.U) + " checkpoint rows of " + std::to_string(wires) +
                                   " wires does not fit the LDS of a workgroup: choose smaller checkpoint_rows");
   }
   return v;
}

// The Variant of a recording's block-start-states kernel, whichever call asks: {P = 1 (stream-major: the rows R of the x-only patch),
// U = the rows of one unrolled group, block}.  ring: as for block_variant -- the scope of the ring backward; without a ring line the
// plain states Variant itself.  With one the value rings are the ring adjoint kernel's LDS bytes, so on time-major frames its
// workgroup; on stream-major buffers R and the block are chosen together: R0 = 2 * states_sm_patch_rows(g), Rmin = max(4, U) (multiples
// of 4 and of U); a graph without input wires declares no patch.  R0 is twice the plain states kernel's -- one stream's run is two
// cache lines, the 256-byte in-run of the forward stream-major long-run bodies: where the rings bound the workgroup anyway the longer
// run costs no occupancy.  Static, not measured against R0 = states_sm_patch_rows(g).
// far: as for block_variant -- the scope of the far backward; without a line deeper than 256 samples the ring states Variant itself.
// With one: FZ_VF_ADJOINT_RING | FZ_VF_ADJOINT_FAR next to FZ_VF_STATES (fz_kernel_states.hip.inc with FZ_FAR), the same U, and the workgroup
// the ring rule gives the graph's LDS ring lines alone, 256 lanes without any -- the far adjoint kernel's.  On stream-major buffers
// (fz_kernel_states_sm.hip.inc with FZ_FAR) the ring rule chooses R and the block together over those LDS ring slots -- none for a
// graph whose deep lines are all far -- and the x-only patch, with the ring call's Rmin and its refusal when nothing fits, and R0 =
// max(states_sm_patch_rows(g), Rmin), HALF the ring states kernel's: the plain states kernel's whole-cache-line run.  A far kernel
// waits on rows in HBM, a load per far read and row, and hides that behind waves rather than behind a longer run (block_variant's
// measured argument for the far adjoint kernel).  Static, not measured against the ring kernel's R0.
static Variant states_variant(const Graph& g, bool ring, bool stream_major, bool far = false)
{
   ring = ring || far;
   require_scope(g, ring, far);
   const RingLayout rl = ring ? ring_layout(g) : RingLayout{};
   const uint32_t slots = rl.slots;
   const bool far_lines = rl.n_fl() != 0;
   Variant v;
   v.P = 1;
   v.U = states_unroll(g);
   v.block = kGradBlock;
   v.flags = FZ_VF_ADJOINT | FZ_VF_STATES | family_bits(slots != 0 || far_lines, stream_major) | (far_lines ? FZ_VF_ADJOINT_FAR : 0u);
   if (slots || (far_lines && stream_major)) {
      const LaneLds lane{slots, stream_major ? g.n_in : 0u, stream_major && g.n_in ? 4u : 0u};
      const uint32_t Rmin = stream_major ? std::max<uint32_t>(4u, v.U) : 1u;
      // (far lines: R0 is half the ring kernel's, see above)
      const uint32_t R0 = !stream_major ? 1u : far_lines ? std::max(states_sm_patch_rows(g), Rmin) : 2 * states_sm_patch_rows(g);
      const RingSmGeometry geo = ring_sm_geometry(lane, R0, Rmin);
      if (!geo.block)                                       // (stream-major only, as above)
         fail(FZ_E_UNSUPPORTED, "stream-major ring recording: the rings of the delay lines deeper than 8 samples (" + std::to_string(slots) + " samples) plus a patch of " +
                                   std::to_string(Rmin) + " rows of " + std::to_string(g.n_in) + " input wires, " + std::to_string(lane.bytes(64, Rmin)) +
                                   " bytes per 64 lanes, do not fit the " + std::to_string(kLdsBytes) + " bytes of LDS of a workgroup");
      v.P = geo.R;
      v.block = geo.block;
   } else if (stream_major) {
      v.P = states_sm_patch_rows(g);                        // (a multiple of U, or shorter than it: then it is the group)
      v.U = std::min(v.U, v.P);
      if (states_sm_patch_bytes(g, v.P) > kLdsBytes)
         fail(FZ_E_UNSUPPORTED, "stream-major recording: a patch of " + std::to_string(v.P) + " rows of " + std::to_string(g.n_in) +
                                   " input wires does not fit the LDS of a workgroup");
   }
   return v;
}

// Could the backward have made v for this graph?  (kernel manifests are data from elsewhere: fz_manifest.cpp asks before it builds)
// The family bits name the maker and its arguments; v fits when that maker, asked for v's own stride, makes exactly v.  So nothing
// fits that no maker makes: another bit, U = 0 (the maker answers with the default stride), a ring bit on a graph without a ring line
// (the makers answer with the plain Variant), the loss next to FZ_VF_STATES.
bool grad_variant_fits(const Graph& g, const Variant& v)
{
   const bool ring = v.flags & FZ_VF_ADJOINT_RING, sm = v.flags & FZ_VF_ADJOINT_SM, loss = v.flags & FZ_VF_ADJOINT_LOSS, far = v.flags & FZ_VF_ADJOINT_FAR;
   try {
      // (the far bit without the ring bit or on a graph without a far line: no maker answers with it; next to FZ_VF_STATES the states
      //  maker answers with its own U, at most 8, never with the loss, and beside the stream-major bit with its own R in P; next to
      //  the stream-major bit the block maker answers with its own R in P: 1, a non-power of two or an R below C is none)
      const Variant w = !(v.flags & FZ_VF_STATES) ? block_variant(g, v.U, ring, sm, loss, far) : states_variant(g, ring, sm, far);
      return w.P == v.P && w.U == v.U && w.block == v.block && w.flags == v.flags;
   } catch (const Error&) {
      return false;                                         // (a graph, a stride or a patch the call refuses)
   }
}

static bool layout_is_stream_major(uint32_t layout)
{
   if (layout != FZ_GRAD_TIME_MAJOR && layout != FZ_GRAD_STREAM_MAJOR) fail(FZ_E_INVALID, "layout must be FZ_GRAD_TIME_MAJOR or FZ_GRAD_STREAM_MAJOR");
   return layout == FZ_GRAD_STREAM_MAJOR;
}

static uint64_t workspace_bytes(const Graph& g, uint64_t n_streams, uint32_t n_samples, uint32_t C)
{
   const uint64_t chunks = ((uint64_t)n_samples + C - 1) / C;
   return chunks * g.n_state * n_streams * 4u;
}

// the ring kernel's workspace: the register rows before every chunk, then the tape -- every row's ring-line source values
// (include/flowz_hip.h: fz_program_ring_grad_workspace states it).  The far kernel's: the far lines are further tape lines, and behind
// the tape lies the adjoint ring, one row per slot of every far line (fz_program_far_grad_workspace states it; a graph without a far
// line has neither)
static uint64_t ring_workspace_bytes(const Graph& g, uint64_t n_streams, uint32_t n_samples, const Variant& v)
{
   if (!(v.flags & FZ_VF_ADJOINT_RING)) return workspace_bytes(g, n_streams, n_samples, v.U);
   const RingLayout rl = ring_layout(g);
   const uint64_t chunks = ((uint64_t)n_samples + v.U - 1) / v.U;
   return (chunks * rl.n_reg() + (uint64_t)n_samples * (rl.n_rl() + rl.n_fl()) + rl.far_slots) * n_streams * 4u;
}

// (the far kernel's two static rules -- which far reads of sweep 1 travel with their chunk's x rows, which path sweep 2 takes -- are
// far_read_with_chunk and far_fast_path in fz_codegen.cpp, next to ring_layout: the code generator writes them into the kernel's
// configuration and links without this file; include/flowz_hip.h states them)

// The rows per block of a recording of T rows (the one home of this rule; include/flowz_hip.h states it).  block_rows == 0: the B that
// minimises the row sets kept, ceil(B / C) + ceil(T / B) -- sqrt(T * C) rounded up to a multiple of lcm(4, C) = max(4, C) (time-major
// blocks are pointer offsets and keep the 16-byte alignment; checkpoint chunks stay whole), and B = T when that is not smaller.
// A block_rows beyond T is one block of T rows.
static uint32_t recording_block_rows(uint32_t T, uint32_t C, uint32_t block_rows)
{
   if (block_rows) return std::min(block_rows, T);
   const uint64_t m = std::max<uint32_t>(4u, C);
   uint64_t B = (uint64_t)std::ceil(std::sqrt((double)T * (double)C));
   while (B * B < (uint64_t)T * C) ++B;                      // (whatever sqrt rounded: B is the least integer with B^2 >= T C)
   B = (B + m - 1) / m * m;
   return B < T ? (uint32_t)B : T;
}

// The rows per block of a recording of a ring graph (the one home of this rule; include/flowz_hip.h states it).  The row sets kept are
// ceil(T / B) n_state of starts, ceil(B / C) n_register_state of checkpoints and B n_ring_lines of tape; block_rows == 0 starts from
// the continuous minimiser of their sum, the least B with B^2 (n_register_state + C n_ring_lines) >= T n_state C, rounded up like
// recording_block_rows.  Without a ring line the rule IS recording_block_rows.
// far: the recording of the far family -- the far lines are further tape lines of a block, B n_far_lines rows more, so they count with
// the ring lines (n_state counts their slots and phase rows: a block start costs D + 1 rows per far line, so the blocks are long);
// the sum of their depths, the adjoint ring, does not depend on B.  Without a far line the rule IS the ring rule.
static uint32_t ring_recording_block_rows(const Graph& g, uint32_t T, uint32_t C, uint32_t block_rows, bool far = false)
{
   const RingLayout rl = ring_layout(g);
   const uint32_t lines = rl.n_rl() + (far ? rl.n_fl() : 0u);
   if (!lines) return recording_block_rows(T, C, block_rows);
   if (block_rows) return std::min(block_rows, T);
   const uint64_t m = std::max<uint32_t>(4u, C), den = (uint64_t)rl.n_reg() + (uint64_t)C * lines, num = (uint64_t)T * g.n_state * C;
   uint64_t B = (uint64_t)std::ceil(std::sqrt((double)num / (double)den));
   while (B && (B - 1) * (B - 1) * den >= num) --B;          // (whatever sqrt rounded: B is the least integer with B^2 den >= num)
   while (B * B * den < num) ++B;
   B = (B + m - 1) / m * m;
   return B < T ? (uint32_t)B : T;
}

// bytes of the block-start states, [ceil(T / B)][n_state][n_streams] floats: the head of a recording's workspace
static uint64_t starts_bytes(const Graph& g, uint64_t n_streams, uint32_t T, uint32_t B) { return (((uint64_t)T + B - 1) / B) * g.n_state * n_streams * 4u; }

// kernarg image of `struct fz_states_args` (fz_kernel_states.hip.inc) up to the coefficient tail; the stream-major text has the
// window (SmWindow) behind it
struct StatesArgsHeader {
   const float* in;
   const float* state;
   const float* params;
   float* starts;
   float* state_out;
   unsigned long long n_streams;
   unsigned int n_samples;
   unsigned int block_rows;
};
static_assert(sizeof(StatesArgsHeader) == 5 * 8 + 8 + 2 * 4, "StatesArgsHeader must match the head of the kernel's fz_states_args without padding");

// kernarg image of `struct fz_adj_args` without FZ_LOSS (fz_kernel_adjoint.hip.inc; the ring text has the same layout) up to the
// coefficient tail; the stream-major texts have the window (SmWindow) behind it
struct AdjArgsHeader {
   const float* in;
   const float* state;
   const float* params;
   const float* out_grad;
   const float* state_grad;
   float* in_grad;
   float* state0_grad;
   float* param_grad;
   float* const_grad;
   float* ckpt;
   unsigned long long n_streams;
   unsigned int n_samples;
   unsigned int n_chunks;
};
static_assert(sizeof(AdjArgsHeader) == 10 * 8 + 8 + 2 * 4, "AdjArgsHeader must match the head of the kernel's fz_adj_args without padding");

// the same with FZ_LOSS: it ends in one float, and the first kAdjLossHeaderBytes of it are what the kernel's struct holds there; the
// stream-major texts have the window behind them
struct AdjLossArgsHeader {
   const float* in;
   const float* state;
   const float* params;
   const float* target;
   const float* state_grad;
   float* in_grad;
   float* state0_grad;
   float* param_grad;
   float* const_grad;
   float* ckpt;
   float* loss;
   float* out;
   unsigned long long n_streams;
   unsigned int n_samples;
   unsigned int n_chunks;
   float grad_scale;
};
constexpr size_t kAdjLossHeaderBytes = offsetof(AdjLossArgsHeader, grad_scale) + sizeof(float);
static_assert(kAdjLossHeaderBytes == 12 * 8 + 8 + 2 * 4 + 4, "AdjLossArgsHeader must match the head of the kernel's fz_adj_args under FZ_LOSS without padding");

// (the window of a stream-major launch, SmWindow: fz_kernargs.hpp; a null one below: time-major frames)

// the arguments of a backward, whichever struct they came in: fz_grad_args gives dL/dy (`ybar`), fz_loss_grad_args the target in its
// place and what the squared-error rule needs (`loss_rule`)
struct GradCall {
   uint32_t checkpoint_rows;
   const float *in, *state, *params, *ybar, *state_grad;
   float *in_grad, *state0_grad, *param_grad, *const_grad;
   void* workspace;
   uint64_t workspace_bytes;
   bool loss_rule;
   float grad_scale;
   float *loss, *out;
   bool ring = false;          // the call is of the ring family (fz_run_block_ring_*, fz_run_recording_ring_*): its scope, Variant and workspace
   bool far = false;           // the call is of the far family (fz_run_block_far_*, fz_run_recording_far_*): a ring call that takes lines deeper than 256 samples too
};

template <class Args>
static const Args* checked_args(fz_program* p, const Args* a, const char* fn, const char* type)
{
   if (!p) fail(FZ_E_INVALID, "null program");
   if (!a) fail(FZ_E_INVALID, std::string(fn) + ": null arguments");
   if (a->struct_size != sizeof(Args))
      fail(FZ_E_INVALID, std::string(type) + ".struct_size is " + std::to_string(a->struct_size) + ", this library knows " + std::to_string(sizeof(Args)));
   return a;
}

static GradCall call_of(fz_program* p, const fz_grad_args* a0)
{
   const fz_grad_args* a = checked_args(p, a0, "fz_run_block_grad", "fz_grad_args");
   return GradCall{a->checkpoint_rows, a->in, a->state, a->params, a->out_grad, a->state_grad, a->in_grad, a->state0_grad, a->param_grad, a->const_grad,
                   a->workspace, a->workspace_bytes, false, 0.f, nullptr, nullptr};
}

static GradCall call_of(fz_program* p, const fz_loss_grad_args* a0)
{
   const fz_loss_grad_args* a = checked_args(p, a0, "fz_run_block_loss_grad", "fz_loss_grad_args");
   return GradCall{a->checkpoint_rows, a->in, a->state, a->params, a->target, a->state_grad, a->in_grad, a->state0_grad, a->param_grad, a->const_grad,
                   a->workspace, a->workspace_bytes, true, a->grad_scale, a->loss, a->out};
}

// the same for a call of the ring family
template <class Args>
static GradCall ring_call_of(fz_program* p, const Args* a)
{
   GradCall call = call_of(p, a);
   call.ring = true;
   return call;
}

// the same for a call of the far family
template <class Args>
static GradCall far_call_of(fz_program* p, const Args* a)
{
   GradCall call = ring_call_of(p, a);
   call.far = true;
   return call;
}

// what a recording adds to the checks of a block: its own workspace size (and the call that answers it), and state_out as one more output
struct RecordingCheck {
   uint64_t need;
   float* state_out;
};

// every argument check of a backward, before a device is needed; false: an empty block (FZ_OK, nothing to launch).  rec: the call is a
// whole recording (fz_run_recording_grad), checked over its T rows.  own_rows: the call is a block launch of a recording, whose `state` and
// `workspace` are the library's own rows of the caller's workspace -- [row][n_streams] rows at offsets of whole rows, read and written
// per lane in 4-byte accesses like the checkpoint rows of any launch, so the 16-byte rule of the caller's pointers is not asked of them
static bool check_grad(fz_program* p, const GradCall& call, uint64_t n_streams, uint32_t n_samples, const SmWindow* sm, Variant* vout,
                       const RecordingCheck* rec = nullptr, bool own_rows = false)
{
   const GradCall* const a = &call;
   const Graph& g = p->g;
   const Variant v = block_variant(g, a->checkpoint_rows, a->ring, sm != nullptr, a->loss_rule, a->far);
   *vout = v;
   if (!block_has_work(n_streams, n_samples)) return false;   // an empty block: nothing to differentiate, nothing touched
   if (sm) {
      check_window(sm->rows_total, sm->row0, n_samples);
      // (the forward stream-major rule, in the words the backward has for it: the buffers' rule first, then the window's)
      if (!on_piece_grid(sm->rows_total, g.n_in) || !on_piece_grid(sm->rows_total, g.n_out))
         fail(FZ_E_INVALID, "stream-major buffers: rows_total * n_in and rows_total * n_out must be multiples of 4 floats");
      if (!on_piece_grid(sm->row0, g.n_in) || !on_piece_grid(sm->row0, g.n_out))
         fail(FZ_E_INVALID, "stream-major buffers: row0 * n_in and row0 * n_out must be multiples of 4 floats");
   }
   check_stream_count(n_streams);
   require_pointer(a->in, g.n_in, "in", "input wires");
   require_pointer(a->state, g.n_state, "state", "delay lines");
   require_pointer(a->params, g.n_param, "params", "per-stream coefficients");
   if (a->loss_rule && !a->ybar) fail(FZ_E_INVALID, "target is null: the loss compares the outputs with it");
   require_pointer(a->ybar, g.n_out, "out_grad", "output wires");
   const uint64_t need = rec ? rec->need : ring_workspace_bytes(g, n_streams, n_samples, v);
   const std::string ws_fn = rec ? (a->far ? "fz_program_far_recording_workspace" : a->ring ? "fz_program_ring_recording_workspace" : "fz_program_recording_workspace") : a->far ? "fz_program_far_grad_workspace" : a->ring ? "fz_program_ring_grad_workspace" : "fz_program_grad_workspace";
   if (need && !a->workspace) fail(FZ_E_INVALID, "workspace is null: " + ws_fn + " says " + std::to_string(need) + " bytes");
   if (need && a->workspace_bytes < need)
      fail(FZ_E_INVALID, "workspace_bytes " + std::to_string(a->workspace_bytes) + " is less than the " + std::to_string(need) + " bytes " + ws_fn + " asks for");
   // (bytes of one wire's frames: a stream-major buffer is touched over its whole extent, n_streams * rows_total rows)
   const uint64_t fr = (uint64_t)(sm ? sm->rows_total : n_samples) * n_streams * 4u, row = n_streams * 4u;
   struct Buf {
      const void* ptr;
      uint64_t bytes;
      const char* name;
      bool out;
      bool own = false;        // one of the library's own rows in a block launch of a recording: no 16-byte rule (see above)
   };
   // (only what the kernel touches: buffers of zero rows are never dereferenced)
   std::vector<Buf> bufs = {
      {a->in, g.n_in ? fr * g.n_in : 0, "in", false},          {a->state, row * g.n_state, "state", false, own_rows},
      {a->params, row * g.n_param, "params", false},           {a->ybar, g.n_out ? fr * g.n_out : 0, a->loss_rule ? "target" : "out_grad", false},
      {a->state_grad, row * g.n_state, "state_grad", false},   {a->in_grad, g.n_in ? fr * g.n_in : 0, "in_grad", true},
      {a->state0_grad, row * g.n_state, "state0_grad", true},  {a->param_grad, row * g.n_param, "param_grad", true},
      {a->const_grad, row * g.consts.size(), "const_grad", true}, {a->workspace, need, "workspace", true, own_rows},
      {a->loss, row, "loss", true},                            {a->out, g.n_out ? fr * g.n_out : 0, "out", true},
   };
   if (rec) bufs.push_back({rec->state_out, row * g.n_state, "state_out", true});
   for (const Buf& b : bufs)
      if (!b.own) check_aligned16({{b.ptr, b.name}});
   for (size_t i = 0; i < bufs.size(); ++i)
      for (size_t j = i + 1; j < bufs.size(); ++j) {
         const Buf &x = bufs[i], &y = bufs[j];
         if (!(x.out || y.out) || !x.ptr || !y.ptr || !x.bytes || !y.bytes) continue;
         if (x.ptr == a->state_grad && y.ptr == a->state0_grad && x.ptr == y.ptr) continue;   // (sbar0 may overwrite sbar_T in place)
         const uintptr_t x0 = reinterpret_cast<uintptr_t>(x.ptr), y0 = reinterpret_cast<uintptr_t>(y.ptr);
         if (x0 < y0 + y.bytes && y0 < x0 + x.bytes) fail(FZ_E_INVALID, std::string(x.name) + " and " + y.name + " overlap");
      }
   return true;
}

// The launch of a kernel of the family (a device is at hand).  Its argument struct is the header image, the window of a stream-major launch
// behind it, then the coefficient tail.
static void launch_family(fz_program* p, const Variant& v, const void* header, size_t header_bytes, const SmWindow* sm, uint64_t n_streams, void* stream)
{
   void* fn = nullptr;
   (void)get_kernel(p, v, &fn);
   KernArgs ka(header_bytes, sm != nullptr, p->g.consts.size());
   ka.set_header(header);
   if (sm) ka.set_window(*sm);
   copy_coefficients(ka, p);
   launch_kernel(fn, (unsigned)((n_streams + v.block - 1) / v.block), v.block, stream, ka);
}

// the launch of a checked backward
static void launch_grad(fz_program* p, const Variant& v, const GradCall& a, uint64_t n_streams, uint32_t n_samples, void* stream, const SmWindow* sm)
{
   float* const ws = static_cast<float*>(a.workspace);
   const unsigned int n_chunks = (unsigned int)((n_samples + (uint64_t)v.U - 1) / v.U);
   if (a.loss_rule) {
      const AdjLossArgsHeader h{a.in, a.state, a.params, a.ybar, a.state_grad, a.in_grad, a.state0_grad, a.param_grad, a.const_grad, ws,
                                a.loss, a.out, (unsigned long long)n_streams, n_samples, n_chunks, a.grad_scale};
      launch_family(p, v, &h, kAdjLossHeaderBytes, sm, n_streams, stream);
   } else {
      const AdjArgsHeader h{a.in, a.state, a.params, a.ybar, a.state_grad, a.in_grad, a.state0_grad, a.param_grad, a.const_grad, ws,
                            (unsigned long long)n_streams, n_samples, n_chunks};
      launch_family(p, v, &h, sizeof h, sm, n_streams, stream);
   }
}

static int run_grad(fz_program* p, const GradCall& call, uint64_t n_streams, uint32_t n_samples, void* stream, const SmWindow* sm = nullptr)
{
   Variant v;
   if (!check_grad(p, call, n_streams, n_samples, sm, &v)) return FZ_OK;
   require_device();
   launch_grad(p, v, call, n_streams, n_samples, stream, sm);
   return FZ_OK;
}

// One launch of the block-start-states kernel over the recording (checked by the caller; n_state > 0).
static void launch_states(fz_program* p, const Variant& v, const GradCall& a, float* starts, float* state_out, uint64_t n_streams, uint32_t n_samples,
                          uint32_t B, void* stream, const SmWindow* sm)
{
   const StatesArgsHeader h{a.in, a.state, a.params, starts, state_out, (unsigned long long)n_streams, n_samples, B};
   launch_family(p, v, &h, sizeof h, sm, n_streams, stream);
}

static uint64_t recording_workspace_bytes(const Graph& g, uint64_t n_streams, uint32_t T, uint32_t B, uint32_t C)
{
   return T ? starts_bytes(g, n_streams, T, B) + workspace_bytes(g, n_streams, B, C) : 0;
}

// the workspace of a ring recording (the one home of this rule): the block-start states, then one block's ring workspace -- v is the
// block launches' Variant; for a graph without a ring line this is recording_workspace_bytes.  The far family's is the same sum with the
// far block Variant (ring_workspace_bytes counts the far lines' tape and adjoint ring then): no rule of its own
static uint64_t ring_recording_workspace_bytes(const Graph& g, uint64_t n_streams, uint32_t T, uint32_t B, const Variant& v)
{
   return T ? starts_bytes(g, n_streams, T, B) + ring_workspace_bytes(g, n_streams, B, v) : 0;
}

// The backward of a recording: the states kernel once, then the block launches from the last block to the first (the contract is in
// include/flowz_hip.h).  Every check -- of the call over its T rows, then of every block launch as a direct call would be checked --
// runs before a device is needed.  call.ring: the recording of the ring family, in either layout -- the scope, the states kernel, B
// and the workspace are that family's, the rest is shared.  call.far: the recording of the far family, in either layout -- the same
// again with the far makers; the far states kernel keeps its working rings in the rows behind `starts`, the head of the block
// workspace, which no block launch has used yet, and the block launches are the far adjoint kernels unchanged.  C, B and the
// workspace do not depend on the layout.
static int run_recording(fz_program* p, const GradCall& call, uint32_t layout, uint64_t n_streams, uint32_t rows_total, uint32_t row0, uint32_t n_samples,
                         uint32_t block_rows, float* state_out, void* stream)
{
   const Graph& g = p->g;
   const bool stream_major = layout_is_stream_major(layout);
   require_scope(g, call.ring, call.far);                  // (scope first: the refusals of fz_program_grad_check, fz_program_ring_grad_check, fz_program_far_grad_check)
   // (a graph without delay lines launches no states kernel: its LDS patch is not asked to fit)
   const Variant sv = !g.n_state ? Variant{} : states_variant(g, call.ring, stream_major, call.far);
   auto rows_per_block = [&](uint32_t C) { return call.ring ? ring_recording_block_rows(g, n_samples, C, block_rows, call.far) : recording_block_rows(n_samples, C, block_rows); };
   if (!stream_major && block_rows % 4)
      fail(FZ_E_INVALID, "block_rows must be a multiple of 4 on time-major frames: the blocks are pointer offsets and keep the 16-byte alignment");
   if (!stream_major && (row0 || (rows_total && rows_total != n_samples)))
      fail(FZ_E_INVALID, "time-major frames have no window: row0 must be 0 and rows_total 0 or n_samples");
   if (n_samples >= (1u << 31)) fail(FZ_E_INVALID, "a recording must be shorter than 2^31 rows");
   const SmWindow whole{rows_total, row0};
   const SmWindow* const sm = stream_major ? &whole : nullptr;
   Variant v;
   {
      // (C is needed for the workspace the checks ask for; block_variant validates checkpoint_rows and the loss's outputs)
      const Variant v0 = block_variant(g, call.checkpoint_rows, call.ring, stream_major, call.loss_rule, call.far);
      const uint32_t B0 = n_samples ? rows_per_block(v0.U) : 0;
      const RecordingCheck rec{call.ring ? ring_recording_workspace_bytes(g, n_streams, n_samples, B0, v0) : recording_workspace_bytes(g, n_streams, n_samples, B0, v0.U), state_out};
      if (!check_grad(p, call, n_streams, n_samples, sm, &v, &rec)) return FZ_OK;
   }
   const uint32_t B = rows_per_block(v.U), nb = (uint32_t)(((uint64_t)n_samples + B - 1) / B);
   if (nb > 1 && g.n_state && !call.state0_grad)
      fail(FZ_E_INVALID, "state0_grad is null: the blocks of a recording chain through it (it may be state_grad)");
   float* const starts = static_cast<float*>(call.workspace);
   const uint64_t sbytes = starts_bytes(g, n_streams, n_samples, B), set = (uint64_t)g.n_state * n_streams;   // floats of one [n_state][n_streams]
   // block k as a call of its own: rows [k B, min((k + 1) B, T)), state = starts[k], the state gradient chained in place
   auto block_call = [&](uint32_t k, SmWindow* w, uint32_t* rows) {
      GradCall b = call;
      *rows = std::min<uint64_t>(B, (uint64_t)n_samples - (uint64_t)k * B);
      const uint64_t off = (uint64_t)k * B * n_streams;     // frames in front of a time-major block, per wire
      if (stream_major) *w = SmWindow{rows_total, row0 + k * B};
      else {
         if (b.in) b.in += off * g.n_in;
         if (b.ybar) b.ybar += off * g.n_out;
         if (b.in_grad) b.in_grad += off * g.n_in;
         if (b.out) b.out += off * g.n_out;
      }
      if (g.n_state) b.state = starts + (uint64_t)k * set;
      if (k + 1 < nb) b.state_grad = call.state0_grad;
      b.workspace = static_cast<char*>(call.workspace) + sbytes;
      b.workspace_bytes = call.workspace_bytes - sbytes;
      return b;
   };
   for (uint32_t k = nb; k-- > 0;) {
      SmWindow w{};
      uint32_t rows = 0;
      Variant vb;
      (void)check_grad(p, block_call(k, &w, &rows), n_streams, rows, stream_major ? &w : nullptr, &vb, nullptr, true);
   }
   require_device();
   if (g.n_state) launch_states(p, sv, call, starts, state_out, n_streams, n_samples, B, stream, sm);
   for (uint32_t k = nb; k-- > 0;) {
      SmWindow w{};
      uint32_t rows = 0;
      const GradCall b = block_call(k, &w, &rows);
      launch_grad(p, v, b, n_streams, rows, stream, stream_major ? &w : nullptr);
   }
   return FZ_OK;
}

}  // namespace fz

using namespace fz;

extern "C" {

int fz_program_grad_check(const fz_program* p)
{
   FZ_GUARD(
      if (!p) fail(FZ_E_INVALID, "null program");
      require_supported(p->g);
      return FZ_OK;)
}

int fz_program_grad_workspace(const fz_program* p, uint64_t n_streams, uint32_t n_samples, uint32_t checkpoint_rows, uint64_t* bytes)
{
   FZ_GUARD(
      if (!p || !bytes) fail(FZ_E_INVALID, "fz_program_grad_workspace: bad arguments");
      require_supported(p->g);
      *bytes = workspace_bytes(p->g, n_streams, n_samples, checkpoint_of(p->g, checkpoint_rows));
      return FZ_OK;)
}

// The inspection calls of every kernel of the family, one FZ_INSPECTION (fz_inspect.hpp) per kernel.
#define FZ_ARG_C uint32_t checkpoint_rows,
#define FZ_ARG_LAYOUT uint32_t layout,
#define FZ_SM layout_is_stream_major(layout)
// (block_variant(g, C, ring, stream-major, loss, far) and states_variant(g, ring, stream-major, far) are the two makers)
FZ_INSPECTION(grad, _for, "fz_program_grad_resources", FZ_ARG_C FZ_ARG_LAYOUT, block_variant(p->g, checkpoint_rows, false, FZ_SM, false))
FZ_INSPECTION(loss_grad, _for, "fz_program_loss_grad_resources_for", FZ_ARG_C FZ_ARG_LAYOUT, block_variant(p->g, checkpoint_rows, false, FZ_SM, true))
FZ_INSPECTION(ring_grad, , "fz_program_ring_grad_resources", FZ_ARG_C, block_variant(p->g, checkpoint_rows, true, false, false))
FZ_INSPECTION(ring_grad, _for, "fz_program_ring_grad_resources_for", FZ_ARG_C FZ_ARG_LAYOUT, block_variant(p->g, checkpoint_rows, true, FZ_SM, false))
FZ_INSPECTION(ring_loss_grad, , "fz_program_ring_loss_grad_resources", FZ_ARG_C, block_variant(p->g, checkpoint_rows, true, false, true))
FZ_INSPECTION(ring_loss_grad, _for, "fz_program_ring_loss_grad_resources_for", FZ_ARG_C FZ_ARG_LAYOUT, block_variant(p->g, checkpoint_rows, true, FZ_SM, true))
FZ_INSPECTION(far_grad, , "fz_program_far_grad_resources", FZ_ARG_C, block_variant(p->g, checkpoint_rows, true, false, false, true))
FZ_INSPECTION(far_loss_grad, , "fz_program_far_loss_grad_resources", FZ_ARG_C, block_variant(p->g, checkpoint_rows, true, false, true, true))
FZ_INSPECTION(far_grad, _for, "fz_program_far_grad_resources_for", FZ_ARG_C FZ_ARG_LAYOUT, block_variant(p->g, checkpoint_rows, true, FZ_SM, false, true))
FZ_INSPECTION(far_loss_grad, _for, "fz_program_far_loss_grad_resources_for", FZ_ARG_C FZ_ARG_LAYOUT, block_variant(p->g, checkpoint_rows, true, FZ_SM, true, true))
FZ_INSPECTION(states, , "fz_program_states_resources", FZ_ARG_LAYOUT, states_variant(p->g, false, FZ_SM))
FZ_INSPECTION(ring_states, , "fz_program_ring_states_resources", , states_variant(p->g, true, false))
FZ_INSPECTION(ring_states, _for, "fz_program_ring_states_resources_for", FZ_ARG_LAYOUT, states_variant(p->g, true, FZ_SM))
FZ_INSPECTION(far_states, , "fz_program_far_states_resources", , states_variant(p->g, true, false, true))
FZ_INSPECTION(far_states, _for, "fz_program_far_states_resources_for", FZ_ARG_LAYOUT, states_variant(p->g, true, FZ_SM, true))
#undef FZ_SM
#undef FZ_ARG_LAYOUT
#undef FZ_ARG_C

int fz_program_grad_resources(fz_program* p, uint32_t checkpoint_rows, fz_kernel_resources* out)
{
   return fz_program_grad_resources_for(p, checkpoint_rows, FZ_GRAD_TIME_MAJOR, out);
}

long fz_program_grad_kernel_symbol(fz_program* p, uint32_t checkpoint_rows, char* buf, size_t cap)
{
   return fz_program_grad_kernel_symbol_for(p, checkpoint_rows, FZ_GRAD_TIME_MAJOR, buf, cap);
}

int fz_run_block_grad(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t n_samples, void* hip_stream)
{
   FZ_GUARD(return run_grad(p, call_of(p, a), n_streams, n_samples, hip_stream);)
}

int fz_run_block_grad_stream_major(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t rows_total, uint32_t row0, uint32_t n_samples,
                                   void* hip_stream)
{
   FZ_GUARD(
      const SmWindow w{rows_total, row0};
      return run_grad(p, call_of(p, a), n_streams, n_samples, hip_stream, &w);)
}

int fz_run_block_loss_grad(fz_program* p, const fz_loss_grad_args* a, uint64_t n_streams, uint32_t n_samples, void* hip_stream)
{
   FZ_GUARD(return run_grad(p, call_of(p, a), n_streams, n_samples, hip_stream);)
}

int fz_run_block_loss_grad_stream_major(fz_program* p, const fz_loss_grad_args* a, uint64_t n_streams, uint32_t rows_total, uint32_t row0,
                                        uint32_t n_samples, void* hip_stream)
{
   FZ_GUARD(
      const SmWindow w{rows_total, row0};
      return run_grad(p, call_of(p, a), n_streams, n_samples, hip_stream, &w);)
}

int fz_program_ring_grad_check(const fz_program* p)
{
   FZ_GUARD(
      if (!p) fail(FZ_E_INVALID, "null program");
      require_scope(p->g, true);
      return FZ_OK;)
}

int fz_program_ring_grad_workspace(const fz_program* p, uint64_t n_streams, uint32_t n_samples, uint32_t checkpoint_rows, uint64_t* bytes)
{
   FZ_GUARD(
      if (!p || !bytes) fail(FZ_E_INVALID, "fz_program_ring_grad_workspace: bad arguments");
      *bytes = ring_workspace_bytes(p->g, n_streams, n_samples, block_variant(p->g, checkpoint_rows, true, false, false));
      return FZ_OK;)
}

int fz_run_block_ring_grad(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t n_samples, void* hip_stream)
{
   FZ_GUARD(return run_grad(p, ring_call_of(p, a), n_streams, n_samples, hip_stream);)
}

int fz_run_block_ring_grad_stream_major(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t rows_total, uint32_t row0, uint32_t n_samples,
                                        void* hip_stream)
{
   FZ_GUARD(
      const SmWindow w{rows_total, row0};
      return run_grad(p, ring_call_of(p, a), n_streams, n_samples, hip_stream, &w);)
}

int fz_run_block_ring_loss_grad_stream_major(fz_program* p, const fz_loss_grad_args* a, uint64_t n_streams, uint32_t rows_total, uint32_t row0,
                                             uint32_t n_samples, void* hip_stream)
{
   FZ_GUARD(
      const SmWindow w{rows_total, row0};
      return run_grad(p, ring_call_of(p, a), n_streams, n_samples, hip_stream, &w);)
}

int fz_run_block_ring_loss_grad(fz_program* p, const fz_loss_grad_args* a, uint64_t n_streams, uint32_t n_samples, void* hip_stream)
{
   FZ_GUARD(return run_grad(p, ring_call_of(p, a), n_streams, n_samples, hip_stream);)
}

int fz_program_far_grad_check(const fz_program* p)
{
   FZ_GUARD(
      if (!p) fail(FZ_E_INVALID, "null program");
      require_scope(p->g, true, true);
      return FZ_OK;)
}

int fz_program_far_grad_workspace(const fz_program* p, uint64_t n_streams, uint32_t n_samples, uint32_t checkpoint_rows, uint64_t* bytes)
{
   FZ_GUARD(
      if (!p || !bytes) fail(FZ_E_INVALID, "fz_program_far_grad_workspace: bad arguments");
      *bytes = ring_workspace_bytes(p->g, n_streams, n_samples, block_variant(p->g, checkpoint_rows, true, false, false, true));
      return FZ_OK;)
}

int fz_run_block_far_grad(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t n_samples, void* hip_stream)
{
   FZ_GUARD(return run_grad(p, far_call_of(p, a), n_streams, n_samples, hip_stream);)
}

int fz_run_block_far_loss_grad(fz_program* p, const fz_loss_grad_args* a, uint64_t n_streams, uint32_t n_samples, void* hip_stream)
{
   FZ_GUARD(return run_grad(p, far_call_of(p, a), n_streams, n_samples, hip_stream);)
}

int fz_run_block_far_grad_stream_major(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t rows_total, uint32_t row0, uint32_t n_samples,
                                       void* hip_stream)
{
   FZ_GUARD(
      const SmWindow w{rows_total, row0};
      return run_grad(p, far_call_of(p, a), n_streams, n_samples, hip_stream, &w);)
}

int fz_run_block_far_loss_grad_stream_major(fz_program* p, const fz_loss_grad_args* a, uint64_t n_streams, uint32_t rows_total, uint32_t row0,
                                            uint32_t n_samples, void* hip_stream)
{
   FZ_GUARD(
      const SmWindow w{rows_total, row0};
      return run_grad(p, far_call_of(p, a), n_streams, n_samples, hip_stream, &w);)
}

int fz_program_far_recording_block_rows(const fz_program* p, uint32_t n_rows, uint32_t block_rows, uint32_t checkpoint_rows, uint32_t* rows)
{
   FZ_GUARD(
      if (!p || !rows) fail(FZ_E_INVALID, "fz_program_far_recording_block_rows: bad arguments");
      const Variant v = block_variant(p->g, checkpoint_rows, true, false, false, true);
      if (n_rows >= (1u << 31)) fail(FZ_E_INVALID, "a recording must be shorter than 2^31 rows");
      *rows = n_rows ? ring_recording_block_rows(p->g, n_rows, v.U, block_rows, true) : 0;
      return FZ_OK;)
}

int fz_program_far_recording_workspace(const fz_program* p, uint64_t n_streams, uint32_t n_rows, uint32_t block_rows, uint32_t checkpoint_rows,
                                       uint64_t* bytes)
{
   FZ_GUARD(
      if (!p || !bytes) fail(FZ_E_INVALID, "fz_program_far_recording_workspace: bad arguments");
      const Variant v = block_variant(p->g, checkpoint_rows, true, false, false, true);
      if (block_rows % 4) fail(FZ_E_INVALID, "block_rows must be a multiple of 4 on time-major frames: the blocks are pointer offsets and keep the 16-byte alignment");
      if (n_rows >= (1u << 31)) fail(FZ_E_INVALID, "a recording must be shorter than 2^31 rows");
      const uint32_t B = n_rows ? ring_recording_block_rows(p->g, n_rows, v.U, block_rows, true) : 0;
      *bytes = ring_recording_workspace_bytes(p->g, n_streams, n_rows, B, v);
      return FZ_OK;)
}

int fz_run_recording_far_grad(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t n_samples, uint32_t block_rows, float* state_out,
                              void* hip_stream)
{
   FZ_GUARD(return run_recording(p, far_call_of(p, a), FZ_GRAD_TIME_MAJOR, n_streams, 0, 0, n_samples, block_rows, state_out, hip_stream);)
}

int fz_run_recording_far_loss_grad(fz_program* p, const fz_loss_grad_args* a, uint64_t n_streams, uint32_t n_samples, uint32_t block_rows,
                                   float* state_out, void* hip_stream)
{
   FZ_GUARD(return run_recording(p, far_call_of(p, a), FZ_GRAD_TIME_MAJOR, n_streams, 0, 0, n_samples, block_rows, state_out, hip_stream);)
}

int fz_run_recording_far_grad_for(fz_program* p, const fz_grad_args* a, uint32_t layout, uint64_t n_streams, uint32_t rows_total, uint32_t row0,
                                  uint32_t n_samples, uint32_t block_rows, float* state_out, void* hip_stream)
{
   FZ_GUARD(return run_recording(p, far_call_of(p, a), layout, n_streams, rows_total, row0, n_samples, block_rows, state_out, hip_stream);)
}

int fz_run_recording_far_loss_grad_for(fz_program* p, const fz_loss_grad_args* a, uint32_t layout, uint64_t n_streams, uint32_t rows_total,
                                       uint32_t row0, uint32_t n_samples, uint32_t block_rows, float* state_out, void* hip_stream)
{
   FZ_GUARD(return run_recording(p, far_call_of(p, a), layout, n_streams, rows_total, row0, n_samples, block_rows, state_out, hip_stream);)
}

int fz_program_ring_recording_block_rows(const fz_program* p, uint32_t n_rows, uint32_t block_rows, uint32_t checkpoint_rows, uint32_t* rows)
{
   FZ_GUARD(
      if (!p || !rows) fail(FZ_E_INVALID, "fz_program_ring_recording_block_rows: bad arguments");
      const Variant v = block_variant(p->g, checkpoint_rows, true, false, false);
      if (n_rows >= (1u << 31)) fail(FZ_E_INVALID, "a recording must be shorter than 2^31 rows");
      *rows = n_rows ? ring_recording_block_rows(p->g, n_rows, v.U, block_rows) : 0;
      return FZ_OK;)
}

int fz_program_ring_recording_workspace(const fz_program* p, uint64_t n_streams, uint32_t n_rows, uint32_t block_rows, uint32_t checkpoint_rows,
                                        uint64_t* bytes)
{
   FZ_GUARD(
      if (!p || !bytes) fail(FZ_E_INVALID, "fz_program_ring_recording_workspace: bad arguments");
      const Variant v = block_variant(p->g, checkpoint_rows, true, false, false);
      if (block_rows % 4) fail(FZ_E_INVALID, "block_rows must be a multiple of 4 on time-major frames: the blocks are pointer offsets and keep the 16-byte alignment");
      if (n_rows >= (1u << 31)) fail(FZ_E_INVALID, "a recording must be shorter than 2^31 rows");
      const uint32_t B = n_rows ? ring_recording_block_rows(p->g, n_rows, v.U, block_rows) : 0;
      *bytes = ring_recording_workspace_bytes(p->g, n_streams, n_rows, B, v);
      return FZ_OK;)
}

int fz_run_recording_ring_grad(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t n_samples, uint32_t block_rows, float* state_out,
                               void* hip_stream)
{
   FZ_GUARD(return run_recording(p, ring_call_of(p, a), FZ_GRAD_TIME_MAJOR, n_streams, 0, 0, n_samples, block_rows, state_out, hip_stream);)
}

int fz_run_recording_ring_loss_grad(fz_program* p, const fz_loss_grad_args* a, uint64_t n_streams, uint32_t n_samples, uint32_t block_rows,
                                    float* state_out, void* hip_stream)
{
   FZ_GUARD(return run_recording(p, ring_call_of(p, a), FZ_GRAD_TIME_MAJOR, n_streams, 0, 0, n_samples, block_rows, state_out, hip_stream);)
}

int fz_run_recording_ring_grad_stream_major(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t rows_total, uint32_t row0,
                                            uint32_t n_samples, uint32_t block_rows, float* state_out, void* hip_stream)
{
   FZ_GUARD(return run_recording(p, ring_call_of(p, a), FZ_GRAD_STREAM_MAJOR, n_streams, rows_total, row0, n_samples, block_rows, state_out, hip_stream);)
}

int fz_run_recording_ring_loss_grad_stream_major(fz_program* p, const fz_loss_grad_args* a, uint64_t n_streams, uint32_t rows_total, uint32_t row0,
                                                 uint32_t n_samples, uint32_t block_rows, float* state_out, void* hip_stream)
{
   FZ_GUARD(return run_recording(p, ring_call_of(p, a), FZ_GRAD_STREAM_MAJOR, n_streams, rows_total, row0, n_samples, block_rows, state_out, hip_stream);)
}

int fz_program_recording_workspace(const fz_program* p, uint64_t n_streams, uint32_t n_rows, uint32_t block_rows, uint32_t checkpoint_rows,
                                   uint32_t layout, uint64_t* bytes)
{
   FZ_GUARD(
      if (!p || !bytes) fail(FZ_E_INVALID, "fz_program_recording_workspace: bad arguments");
      require_supported(p->g);
      if (!layout_is_stream_major(layout) && block_rows % 4) fail(FZ_E_INVALID, "block_rows must be a multiple of 4 on time-major frames: the blocks are pointer offsets and keep the 16-byte alignment");
      if (n_rows >= (1u << 31)) fail(FZ_E_INVALID, "a recording must be shorter than 2^31 rows");
      const uint32_t C = checkpoint_of(p->g, checkpoint_rows), B = n_rows ? recording_block_rows(n_rows, C, block_rows) : 0;
      *bytes = recording_workspace_bytes(p->g, n_streams, n_rows, B, C);
      return FZ_OK;)
}

int fz_program_recording_block_rows(const fz_program* p, uint32_t n_rows, uint32_t block_rows, uint32_t checkpoint_rows, uint32_t* rows)
{
   FZ_GUARD(
      if (!p || !rows) fail(FZ_E_INVALID, "fz_program_recording_block_rows: bad arguments");
      require_supported(p->g);
      if (n_rows >= (1u << 31)) fail(FZ_E_INVALID, "a recording must be shorter than 2^31 rows");
      *rows = n_rows ? recording_block_rows(n_rows, checkpoint_of(p->g, checkpoint_rows), block_rows) : 0;
      return FZ_OK;)
}

int fz_run_recording_grad(fz_program* p, const fz_grad_args* a, uint32_t layout, uint64_t n_streams, uint32_t rows_total, uint32_t row0,
                          uint32_t n_samples, uint32_t block_rows, float* state_out, void* hip_stream)
{
   FZ_GUARD(return run_recording(p, call_of(p, a), layout, n_streams, rows_total, row0, n_samples, block_rows, state_out, hip_stream);)
}

int fz_run_recording_loss_grad(fz_program* p, const fz_loss_grad_args* a, uint32_t layout, uint64_t n_streams, uint32_t rows_total, uint32_t row0,
                               uint32_t n_samples, uint32_t block_rows, float* state_out, void* hip_stream)
{
   FZ_GUARD(return run_recording(p, call_of(p, a), layout, n_streams, rows_total, row0, n_samples, block_rows, state_out, hip_stream);)
}

}  // extern "C"
