// Internal structures of libflowz_hip: expression trees, the lowered per-sample DAG, programs.
#pragma once

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "flowz_hip.h"

namespace fz {

// ---- error plumbing -------------------------------------------------------------------------
void set_error(const std::string& msg);
struct Error {
   int code;
   std::string msg;
};
[[noreturn]] void fail(int code, const std::string& msg);

// the body of an extern "C" entry point that returns a code: what it throws becomes the code, the message goes to fz_last_error
#define FZ_GUARD(...)                                                           \
   try { __VA_ARGS__ }                                                                 \
   catch (const fz::Error& er) { fz::set_error(er.msg); return er.code; }       \
   catch (const std::exception& ex) { fz::set_error(ex.what()); return FZ_E_INVALID; }

// a string result of an inspection call: its length, and as much of it as fits `cap` (NUL-terminated) in `buf`; an error: its code
// (negative), the message in fz_last_error
template <class Text>
long string_result(char* buf, size_t cap, Text text)
{
   try {
      const std::string s = text();
      if (buf && cap) {
         const size_t n = std::min(cap - 1, s.size());
         std::memcpy(buf, s.data(), n);
         buf[n] = 0;
      }
      return (long)s.size();
   } catch (const Error& er) {
      set_error(er.msg);
      return er.code;
   }
}

// ---- argument rules of the launches: each written once, all of them checked before a device is needed ----------
// an empty block is nothing to do (false: FZ_OK, nothing touched)
inline bool block_has_work(uint64_t n_streams, uint32_t n_samples)
{
   if (n_streams == 0 || n_samples == 0) return false;
   if (n_samples == 0xFFFFFFFFu) fail(FZ_E_INVALID, "n_samples must be below 2^32 - 1");
   return true;
}
// (state and coefficient rows go through one-row buffer descriptors: 32-bit byte offsets and sizes, n_streams * 4 < 2^32)
inline void check_stream_count(uint64_t n_streams) { if (n_streams >= (1ull << 30)) fail(FZ_E_UNSUPPORTED, "2^30 streams or more per launch: shard the streams"); }
// a pointer the graph needs: "<name> is null but the graph has <what>"
inline void require_pointer(const void* q, bool needed, const char* name, const char* what) { if (needed && !q) fail(FZ_E_INVALID, std::string(name) + " is null but the graph has " + what); }
// device pointers are 16-byte aligned (a null one is); a name goes in front of the refusal
struct NamedPointer {
   const void* ptr;
   const char* name = nullptr;
};
inline void check_aligned16(std::initializer_list<NamedPointer> ptrs)
{
   for (const NamedPointer& q : ptrs)
      if (reinterpret_cast<uintptr_t>(q.ptr) & 15u)
         fail(FZ_E_INVALID, (q.name ? std::string(q.name) + ": " : std::string()) + "device pointers must be 16-byte aligned");
}
// the window [row0, row0 + n_samples) lies inside the rows_total rows of the buffers
inline void check_window(uint32_t rows_total, uint32_t row0, uint32_t n_samples)
{
   if ((uint64_t)row0 + n_samples > rows_total)
      fail(FZ_E_INVALID, "the window [row0, row0 + n_samples) = [" + std::to_string(row0) + ", " + std::to_string((uint64_t)row0 + n_samples) +
                            ") reaches beyond rows_total = " + std::to_string(rows_total));
}
// The piece grid of stream-major rows: every stream's buffer (rows_total x wires samples) and the window's first row (row0 x wires)
// start on the 16-byte pieces the kernels move -- 4 floats or 8 int16 samples.  on_piece_grid is the rule, check_piece_grid one
// side's refusal in words that name the side.
inline uint32_t piece_samples(bool i16) { return i16 ? 8u : 4u; }
inline bool on_piece_grid(uint32_t rows, uint32_t wires, bool i16 = false) { return ((uint64_t)rows * wires) % piece_samples(i16) == 0; }
inline void check_piece_grid(const char* side, uint32_t wires, uint32_t rows_total, uint32_t row0, bool i16)
{
   if (!on_piece_grid(rows_total, wires, i16) || !on_piece_grid(row0, wires, i16))
      fail(FZ_E_INVALID, std::string(side) + ": rows_total x wires and row0 x wires must be multiples of " + std::to_string(piece_samples(i16)) + " on " +
                            (i16 ? "an int16" : "a float32") + " side (16-byte pieces)");
}

// ---- expression tree (the EDSL surface, flowz.hpp:68-93) ---------------------------------------
enum class EK : uint8_t { Placeholder, Delayed, Literal, Uniform, Param, Arith, Neg, Channel, Parallel, Sequence, Feedback, Modulator,
                          Fn1 };   // Fn1: a unary graph function (op = FZ_OP_ABS .. FZ_OP_TANH, FZ_OP_SIN .. FZ_OP_LOG); min / max are Arith nodes

}  // namespace fz

struct fz_expr {
   std::atomic<int> refs{1};
   fz::EK kind;
   uint32_t i = 0;        // placeholder index / param index
   uint32_t n = 0;        // delay
   float value = 0.f;     // literal
   double value64 = 0.0;  // float64 literal
   bool f64 = false;      // literal is a C++ double
   bool cplx = false;     // literal is a std::complex<float> (value, value_im)
   float value_im = 0.f;
   double value64_im = 0.0; // imaginary part of a std::complex<double> literal (cplx && f64)
   fz_op op = FZ_OP_ADD;  // arith
   fz_expr* a = nullptr;
   fz_expr* b = nullptr;
   int in_arity = 0;
   int out_arity = 1;
};

namespace fz {

// an expression as text and back (fz_expr.cpp): what a kernel manifest records of a program
std::string serialize_expr(const fz_expr* root);
fz_expr* parse_expr(const std::string& text);

// stage packing (fz_split.cpp): the graph is K isomorphic segments in series; segment j runs at
// time t-j and segments 2i, 2i+1 share one packed float2 operation per node
struct PackedLine {
   std::vector<uint32_t> srcs;   // per segment: the source node of this delay line
   uint32_t depth;
   uint32_t frame = 0;           // the sub-atom in whose time frame this copy of the line lives (its readers' sub-atom)
};
struct StageSplit {
   bool ok = false;
   uint32_t K = 0;                                  // number of segments (even)
   std::vector<uint32_t> cuts;                      // c_0 = input node ... c_K = output node
   std::vector<std::vector<uint32_t>> tuples;       // per node of segment 0: its partner in every segment, evaluation order
   // Sub-atoms (round 3): every segment is itself cut at m - 1 internal wires into m ATOMS in series (a DF1 biquad: its
   // feed-forward sum and its recursion), and atom a of segment j runs at time t - (j * m + a).  The atoms of a step are then
   // independent of each other: twice the instruction-level parallelism, dependent chains half as long -- what a wave that
   // carries a single packed pair of segments (the parts of a wave split) needs to stop waiting for its own results.
   // The packed value of an internal cut travels to the next atom through a carry register, one step later.
   uint32_t m = 1;                                  // atoms per segment
   std::vector<uint32_t> sub;                       // per tuple: its atom (0 .. m-1); leaves (constants, parameters): the reader's
   std::vector<std::vector<uint32_t>> icuts;        // icuts[a-1]: the tuple whose value crosses from atom a-1 into atom a (a = 1 .. m-1)
   uint32_t atoms() const { return K * m; }         // skewed units in series = masked steps at either end of a block + 1
   std::vector<PackedLine> lines;
   std::vector<uint32_t> prefix;                    // scalar prefix (nodes cuts[0] depends on), evaluation order
   std::vector<uint32_t> prefix_lines;              // delay lines private to the prefix (indices into Graph::lines)
   std::vector<uint32_t> suffix;                    // scalar suffix (what the output makes of the chain's end wire), evaluation order
   std::vector<uint32_t> suffix_lines;              // delay lines private to the suffix
};

// ---- lowered DAG ---------------------------------------------------------------------------------
struct Node {
   uint32_t kind;   // fz_ir_kind
   uint32_t a = 0, b = 0, c = 0;
   float value = 0.f;
   bool f64 = false;   // the node's arithmetic type is double (a double literal is among its ancestors)
   double value64 = 0.0;
};

struct Line {
   uint32_t src;     // node whose value is pushed every sample
   uint32_t depth;   // deepest delayed read
   uint32_t row0;    // first state row
   bool f64 = false; // typed programs: the line stores doubles (two float rows per slot)
   uint8_t part = 0; // typed programs: 1 / 2 = the real / imaginary part of a std::complex<float> wire
   bool in_lds;      // ring buffer in LDS instead of registers
   uint32_t lds_slot0 = 0, lds_size = 0;   // ring placement (size is a power of two >= depth)
   // FAR lines (depth > kLdsMaxDepth): the line's state rows ARE a ring buffer in HBM, written
   // every sample and read `n` samples later through the prefetch path; one extra state row holds
   // the ring phase.  Reads with n <= kRegMaxDepth use `shadow` register copies of the newest values.
   bool far = false;
   uint32_t phase_row = 0;
   uint32_t shadow = 0;
};

struct FarRead {
   uint32_t line;   // index into Graph::lines
   uint32_t n;      // delay
};

struct Graph {
   uint32_t n_in = 0, n_out = 0, n_param = 0;   // n_in / n_out: frame SLOTS (floats per frame)
   uint32_t n_mod = 0;               // sample-rate modulators (fz_modulator)
   bool typed = false;               // fz_compile_typed: wire types carried through inputs, state and outputs
   uint32_t ref_divergent = 0;       // != 0: a feedback the SHIPPED reference evaluates against its own arity table (fz_info.differs_from_reference)
   uint32_t sym_tag = 0;             // low 32 bits of graph_structure_hash: the "_g<tag>" of the kernel symbols (kernel_symbol)
   std::vector<uint8_t> in_dtype;    // per input wire: fz_dtype
   std::vector<Node> nodes;          // topological order
   std::vector<uint32_t> outputs;    // node ids, one per output frame slot
   std::vector<uint8_t> out_part;    // per slot: 0 real wire, 1 / 2 = re / im of a complex wire, 3 / 4 = low / high word of a double (typed)
   uint32_t n_out_wires = 0;         // output_arity (complex wires take two slots)
   std::vector<Line> lines;          // ordered by src
   std::vector<float> consts;        // uniform coefficient slots
   std::vector<double> consts64;     // float64 literal terminals
   std::map<uint32_t, uint32_t> uniform_slot;   // fz_uniform id -> coefficient slot (never shared)
   uint32_t n_state = 0, max_delay = 0, n_ops = 0, n_lds_slots = 0;
   // n_ops weighted by what a node costs in instructions, for the planner's thresholds: 1 for every operator (so the plans of graphs
   // without functions stay what they were), more for the graph functions (fn_weight in fz_lower.cpp)
   uint32_t op_weight = 0;
   std::vector<int> line_of_node;    // node -> line index or -1
   StageSplit split;                 // stage packing, when the graph allows it
   std::vector<FarRead> far_reads;   // distinct (far line, delay) pairs, in first-use order
   std::vector<uint32_t> far_lines;  // indices of far lines
   uint32_t far_min_read = 0;        // smallest delay read from a far line's HBM ring (> kRegMaxDepth); 0: none
   // Wave split (FZ_VF_WAVES(W)): the W parts of a serial graph cut at wires of its stage split, each a graph of its own
   // (1 in, 1 out; constants and state rows are the parent's) that one wave of a W-tuple evaluates.  wave_splits[W] for
   // W = 2, 3, 4; empty when the graph does not allow it.
   std::vector<std::vector<Graph>> wave_splits;
   // (W = 1: the graph itself, when it is stage-packable -- the compute wave next to an I/O wave)
   const std::vector<Graph>* wave_roles(uint32_t W) const { return W && W < wave_splits.size() && wave_splits[W].size() == W ? &wave_splits[W] : nullptr; }
};

// max_atoms: upper bound for K * m (the wave-split hand-offs and the long-run stream-major body bound the total skew)
// force_atoms: cut every segment into atoms even when the chain has three or more packed pairs (a wave that carries ONE pair needs them)
StageSplit find_stage_split(const Graph& g, bool plain = false, uint32_t divisor = 0, uint32_t max_atoms = 13, bool force_atoms = false);
std::vector<Graph> find_wave_roles(const Graph& g, uint32_t W);   // fz_split.cpp; {} or W graphs
// the operation kinds stage packing takes (ADD, SUB, MUL, DIV, NEG: a packed float pair has an instruction for each): fz_split.cpp
bool is_arith(uint32_t kind);
// number of waves per stream tuple a variant asks for (flags bits 10..11: 1024 -> 2, 2048 -> 3, 3072 -> 4), 0 = no wave split
inline uint32_t wave_split_of(uint32_t flags) { const uint32_t b = (flags >> 10) & 3u; return b ? b + 1 : 0; }
// FZ_VF_IO_WAVE: one more wave per tuple does the frame I/O.  Parts of the graph a tuple's compute waves evaluate (0: the ordinary
// kernels), and waves per tuple
inline uint32_t ws_io(uint32_t flags) { return (flags & FZ_VF_IO_WAVE) ? 1u : 0u; }
inline uint32_t ws_parts(uint32_t flags) { const uint32_t W = wave_split_of(flags); return W ? W : ws_io(flags); }
inline uint32_t ws_io_waves(uint32_t flags) { return ws_io(flags) ? ((flags & FZ_VF_IO_WAVE2) ? 2u : 1u) : 0u; }   // FZ_VF_IO_WAVE2: loader and storer are two waves
inline uint32_t ws_waves(uint32_t flags) { return ws_parts(flags) + (ws_parts(flags) ? ws_io_waves(flags) : 0u); }

// variant flag bits that mean nothing (any more): rounds 1-5 kept experiment knobs there (plain loads / block order, the SLP vectoriser, cache
// policies, the persistent launch) -- compile-time switches of the kernel source now (FLOWZ_HIP_EXTRA_OPTS=-DFZ_DBG_...).  Refused by check_request.
constexpr uint32_t FZ_VF_RESERVED = 1u | 2u | 4u | (7u << 12) | (7u << 16) | (1u << 27);
// internal variant flag: the stream count is not a multiple of the streams per lane -- the last lane's accesses run past the rows' ends,
// where the per-row buffer descriptors return zeros / drop the writes (frame kernel in lockstep, plain time-major rows)
constexpr uint32_t FZ_VF_RAGGED = 1u << 28;
// internal: output rows of plain time-major frames that do not start on the store grid (kStoreGridBytes): neighbouring waves share the
// sectors / lines at the ends of their footprints, and the frame stores must let L2 merge them (nt instead of nt | sc1; set by
// fit_variant, profiles/r04/rows_off_the_grid_store_policy.txt)
constexpr uint32_t FZ_VF_ST_MERGE = 1u << 29;
// internal: four streams per lane as TWO PAIRS 128 streams apart (the wave still covers 256 adjacent streams): frames whose lane slice
// would leave in two 16-byte stores -- typed frames of 8 bytes per stream -- then store whole 32-byte sectors per instruction (lanes'
// 16-byte pieces side by side) and can be written through like every other frame (fz_block_kernel.hip.inc: FZ_PAIRS; set by fit_variant)
constexpr uint32_t FZ_VF_LANE_PAIRS = 1u << 30;
// internal: ... as SINGLE streams 64 apart (two or four streams per lane of frames with four floats per stream: every 16-byte access of a
// lane is one stream's frame, contiguous across the lanes of the wave)
constexpr uint32_t FZ_VF_LANE_SINGLES = 1u << 31;
// internal: the ADJOINT kernel of a block (fz_grad.cpp, fz_kernel_adjoint.hip.inc): a reserved bit, so that no caller's variant names
// it.  Such a Variant is {P = 1, U = checkpoint rows, block = lanes per workgroup, flags = FZ_VF_ADJOINT}; it shares the kernel cache
// with the forward kernels (its own source is its key) and none of the forward planner's paths ever sees it.
constexpr uint32_t FZ_VF_ADJOINT = 1u << 27;
// internal, with FZ_VF_ADJOINT: the adjoint kernel for STREAM-MAJOR buffers (fz_kernel_adjoint_sm.hip.inc), a text and a symbol of its
// own; one of the reserved bits, so no caller's variant names it either.  Such a Variant carries the rows of its LDS patch in P
// (fz_grad.cpp: grad_sm_patch_rows is their one home; the kernel itself runs one stream per lane).
constexpr uint32_t FZ_VF_ADJOINT_SM = 1u << 18;
// internal, with FZ_VF_ADJOINT (and optionally FZ_VF_ADJOINT_SM): the adjoint kernel that forms dL/dy itself, from a target and the
// squared-error rule of fz_run_block_loss_grad (the plain kernel's text with FZ_LOSS, a symbol of its own); one more of the reserved
// bits.  P, U and block mean what they mean for the plain adjoint variant.
constexpr uint32_t FZ_VF_ADJOINT_LOSS = 1u << 17;
// internal, with FZ_VF_ADJOINT (and optionally FZ_VF_ADJOINT_SM): the BLOCK-START-STATES kernel of a recording (fz_grad.cpp:
// fz_run_recording_grad; fz_kernel_states.hip.inc, fz_kernel_states_sm.hip.inc: one text per layout, symbols of their own), the forward
// half of the adjoint body alone; one more of the reserved bits.  Such a Variant is {P = 1 (stream-major: the rows of its LDS patch),
// U = the rows of one unrolled group, block = lanes per workgroup}; fz_grad.cpp: states_variant is the one place that makes one.
constexpr uint32_t FZ_VF_STATES = 1u << 16;
// internal, with FZ_VF_ADJOINT: the adjoint kernel of a graph with delay lines in LDS (fz_grad.cpp: fz_run_block_ring_grad;
// fz_kernel_adjoint_ring.hip.inc: a text and a symbol of its own, the pending adjoints of the deep lines in an LDS ring); the last of
// the reserved bits 12 .. 14 that nothing used, so a forward variant naming it stays refused as reserved.  Such a Variant is {P = 1,
// U = checkpoint rows, block = 256 / 128 / 64 lanes per workgroup}; fz_grad.cpp: block_variant is the one place that makes one.
// With FZ_VF_ADJOINT_LOSS next to it: the ring kernel that forms dL/dy itself (fz_run_block_ring_loss_grad: the ring kernel's text
// with FZ_LOSS, one more symbol), the same P, U and block.
// With FZ_VF_ADJOINT_SM next to it (with or without FZ_VF_ADJOINT_LOSS): the ring kernels for STREAM-MAJOR buffers
// (fz_run_block_ring_grad_stream_major, fz_run_block_ring_loss_grad_stream_major; fz_kernel_adjoint_ring_sm.hip.inc: a text of
// its own, a symbol each), {P = rows of the LDS patch, U = the ring kernel's checkpoint
// rows, block = 256 / 128 / 64}: rings and patches share the workgroup's LDS, so fz_grad.cpp: ring_sm_geometry chooses P and block
// together and block_variant is the one place that makes one.
// With FZ_VF_STATES next to it (never FZ_VF_ADJOINT_LOSS): the block-start-states kernel of a ring recording
// (fz_run_recording_ring_grad; fz_kernel_states.hip.inc with FZ_RING, a symbol of its own), {P = 1, U = the rows of one unrolled
// group, block = the ring adjoint kernel's}; fz_grad.cpp: states_variant is the one place that makes one.
// With FZ_VF_STATES and FZ_VF_ADJOINT_SM next to it: the same for STREAM-MAJOR buffers (fz_run_recording_ring_grad_stream_major;
// fz_kernel_states_sm.hip.inc with FZ_RING, a symbol of its own), {P = rows of the x-only LDS patch, U = the rows of one unrolled
// group, block = 256 / 128 / 64}: fz_grad.cpp: ring_sm_geometry chooses P and block together and states_variant is the one place that
// makes one.
constexpr uint32_t FZ_VF_ADJOINT_RING = 1u << 14;
// internal, with FZ_VF_ADJOINT | FZ_VF_ADJOINT_RING (optionally FZ_VF_ADJOINT_LOSS): the
// adjoint kernel of a graph with delay lines DEEPER THAN 256 SAMPLES, whose rings live in HBM (fz_grad.cpp: fz_run_block_far_grad,
// fz_run_block_far_loss_grad; fz_kernel_adjoint_ring.hip.inc with FZ_FAR: the ring text, a symbol of its own, the pending adjoints of the far lines
// in a ring in the workspace).  The flag 1u is one of the reserved ones -- a forward variant naming it stays refused -- and the flags
// 1u, 2u and 4u otherwise mean something next to FZ_VF_PCM16 only (FZ_VF_PCM16_IN / _OUT / _B16 below); next to FZ_VF_ADJOINT 1u is this.
// Such a Variant is {P = 1, U = checkpoint rows, block = the ring rule's answer for the graph's LDS ring lines alone, 256 without
// any}; fz_grad.cpp: block_variant is the one place that makes one, and only for a graph that has a far line.
// With FZ_VF_ADJOINT_SM next to the two (with or without FZ_VF_ADJOINT_LOSS): the far kernels for STREAM-MAJOR buffers
// (fz_run_block_far_grad_stream_major, fz_run_block_far_loss_grad_stream_major; fz_kernel_adjoint_ring_sm.hip.inc with FZ_FAR),
// {P = the patch rows R, U = checkpoint rows, block}: the stream-major ring rule over the LDS ring lines alone, from half its R0.
// With FZ_VF_STATES next to the two (never FZ_VF_ADJOINT_LOSS or FZ_VF_ADJOINT_SM): the block-start-states kernel of a far recording
// (fz_run_recording_far_grad; fz_kernel_states.hip.inc with FZ_RING and FZ_FAR: a symbol of its own, the far lines' values in a working ring in
// the workspace), {P = 1, U = the rows of one unrolled group, at most 8, block = the far adjoint kernel's}; fz_grad.cpp:
// states_variant is the one place that makes one, and only for a graph that has a far line.
constexpr uint32_t FZ_VF_ADJOINT_FAR = 1u;
// internal: the kernel for 16-bit PCM frames (fz_pcm16.cpp, fz_kernel_pcm16.hip.inc), one of the reserved bits -- no caller's variant
// names it -- and, meaningful with it only, three more: `in` is int16, `out` is int16, the int16 rows are off the dword grid (2-byte
// accesses).  FZ_VF_ST_MERGE means for it what it means for the frame kernel.  Such a Variant shares the kernel cache and the manifests
// with every other; the forward planner never sees it (fz_pcm16.cpp: pcm16_plan is the one place that makes one).
constexpr uint32_t FZ_VF_PCM16 = 1u << 12;
constexpr uint32_t FZ_VF_PCM16_IN = 1u, FZ_VF_PCM16_OUT = 2u, FZ_VF_PCM16_B16 = 4u;
// internal, with FZ_VF_PCM16: the PCM kernel for STREAM-MAJOR buffers (fz_kernel_pcm16_sm.hip.inc), a text and a symbol of its own; one
// more of the reserved bits.  Such a Variant is {P = 1, U = rows per chunk, block = 64, flags = these two + the IN / OUT bits}
// (fz_pcm16.cpp: pcm16_sm_chunk_rows is the one home of U).
constexpr uint32_t FZ_VF_PCM16_SM = 1u << 13;
// internal: the FORWARD kernel for stream-major float32 buffers of a graph with delay lines deeper than 256 samples, rings in HBM
// (fz_far_sm.cpp: fz_run_block_far_stream_major; fz_kernel_far_sm.hip.inc behind the common head, a text and a symbol of its own).
// Its flag set is the two reserved bits that read "stream-major, far" WITHOUT FZ_VF_ADJOINT, and exactly those: no maker of the
// adjoint family produces it (each sets bit 27), no caller's variant names it (check_request refuses both bits).  Such a Variant is
// {P = the patch rows R, U = the rows G of one unrolled group, block = lanes per workgroup}; codegen puts R into FZ_R and compiles
// the body for one stream per lane.  fz_far_sm.cpp: far_sm_plan is the one place that makes one.
constexpr uint32_t FZ_VF_FAR_SM = FZ_VF_ADJOINT_SM | FZ_VF_ADJOINT_FAR;
inline bool is_far_sm(uint32_t flags) { return flags == FZ_VF_FAR_SM; }
constexpr uint32_t kChipCUs = 256;       // MI355X (gfx950): 8 XCDs x 32 CUs -- what chip_cus() answers on a box without a GPU
unsigned chip_cus();                     // compute units of the current device (fz_launch.cpp)

// register-resident delay lines up to this depth; deeper ones become LDS rings
constexpr uint32_t kRegMaxDepth = 8;
constexpr uint32_t kLdsMaxDepth = 256;   // deeper lines live in HBM (ring in the state buffer)
constexpr uint32_t kFarMinDelay = 32;    // far reads at least this old allow the full 16-step prefetch chunk (a read must be two chunks old)

struct LowerOptions {
   bool typed = false;               // ResultType semantics for inputs, state and outputs
   std::vector<uint8_t> in_dtype;    // per input wire (typed only); missing entries: float
};
Graph lower(const fz_expr* e, const LowerOptions& opt = LowerOptions());   // throws Error
std::vector<uint32_t> max_input_delays(const fz_expr* e);
uint32_t feedback_promise_inputs(const fz_expr* fb);   // fz_expr.cpp; SURVEY App. C.1

// ---- code generation -------------------------------------------------------------------------------
struct Variant {
   uint32_t P = 2, U = 8, block = 256, flags = 0;
   bool operator<(const Variant& o) const {
      if (P != o.P) return P < o.P;
      if (U != o.U) return U < o.U;
      if (block != o.block) return block < o.block;
      return flags < o.flags;
   }
};

std::string kernel_name(const Graph& g, const Variant& v);     // the variant: fz_block_kernel_p<P>u<U>b<block>...f<flags>
std::string kernel_symbol(const Graph& g, const Variant& v);   // the symbol in the code object: kernel_name + "_g<graph tag>"
// how a frame kernel keeps its LDS rings (fz_codegen.cpp: ring_plan): vectorised in time where the graph allows
struct RingPlan {
   bool vec = false;          // lane-major rows, 16-byte accesses of 4 / P time steps, reads fetched / pushes flushed per sub-chunk
   uint32_t G = 0;            // steps per sub-chunk
   uint32_t TW = 1;           // time steps per 16-byte access
   uint32_t pad = 0;          // padding slots per lane and line
   uint32_t lane_floats = 0;  // floats per lane of all rings
   uint32_t slots = 0;        // V slots per lane the kernel declares (FZ_LDS_SLOTS)
};
RingPlan ring_plan(const Graph& g, const Variant& v);
std::string gen_config(const Graph& g, const Variant& v); // generated "fz_graph_config.h"
std::string gen_body(const Graph& g, const Variant& v);   // generated "fz_graph_body.h"
const std::string& skeleton_source(const Variant& v);   // hand-written kernel text of a variant: the common head + the one body it selects
std::string full_source(const Graph& g, const Variant& v);
// the adjoint kernel (a Variant with FZ_VF_ADJOINT): gen_config / gen_body / skeleton_source hand over to these for it
std::string gen_adjoint_config(const Graph& g, const Variant& v);
// loss: also out(), the step's output values (FZ_VF_ADJOINT_LOSS).  ring: the body of fz_kernel_adjoint_ring.hip.inc (FZ_VF_ADJOINT_RING):
// register rows compact, the lines in LDS read through rv[] and their adjoints kept in an LDS ring; without it the text is unchanged.
// Both: out() takes rv[] too (fz_kernel_adjoint_ring.hip.inc with FZ_LOSS)
// far (FZ_VF_ADJOINT_FAR, with ring): the body of fz_kernel_adjoint_ring.hip.inc with FZ_FAR -- the far lines' reads follow the ring reads in
// rv[], their source values the ring lines' in u[]; 1: bwd() keeps their pending adjoints in the workspace ring (the per-row path),
// 2: in the registers the kernel hands it (the fast path); fz_codegen.cpp: far_fast_path chooses
std::string gen_adjoint_body(const Graph& g, bool loss = false, bool ring = false, int far = 0);
// How the ring adjoint kernel lays a graph out (fz_codegen.cpp; the one home of these counts for fz_grad.cpp too): the lines of depth
// <= 8 keep compact REGISTER rows, every `in_lds` line is a RING LINE with its slots in the lane's LDS column, and the distinct
// (ring line, delay) pairs the graph reads are the RING READS, in node order.
struct RingLayout {
   std::vector<int> reg0;            // per line: its first compact register row, -1 for a ring line
   std::vector<int> ring_of_line;    // per line: its ring line index, -1 for a register line
   std::vector<uint32_t> reg_row;    // per compact register row: the caller's state row
   std::vector<uint32_t> rl_line;    // per ring line: index into Graph::lines
   std::vector<uint32_t> rl_slot0;   // per ring line: its first LDS slot
   std::vector<std::pair<uint32_t, uint32_t>> reads;   // (ring line, delay)
   uint32_t slots = 0;               // LDS slots per lane: the sum of the ring lines' depths
   // the FAR lines (Line::far, deeper than 256 samples: FZ_FAR in fz_kernel_adjoint_ring.hip.inc), neither register rows nor ring lines
   std::vector<int> far_of_line;     // per line: its far line index, -1 for any other line
   std::vector<uint32_t> fl_line;    // per far line: index into Graph::lines
   std::vector<uint32_t> fl_slot0;   // per far line: its first row of the adjoint ring in the workspace
   std::vector<std::pair<uint32_t, uint32_t>> far_reads;   // (far line, delay), in node order
   uint32_t far_slots = 0;           // rows of the adjoint ring in the workspace: the sum of the far lines' depths
   uint32_t n_reg() const { return (uint32_t)reg_row.size(); }
   uint32_t n_rl() const { return (uint32_t)rl_line.size(); }
   uint32_t n_rr() const { return (uint32_t)reads.size(); }
   uint32_t n_fl() const { return (uint32_t)fl_line.size(); }
   uint32_t n_fr() const { return (uint32_t)far_reads.size(); }
   int read_index(uint32_t ring_line, uint32_t delay) const;   // -1: no such read
   int far_read_index(uint32_t far_line, uint32_t delay) const;   // -1: no such read
};
RingLayout ring_layout(const Graph& g);
// the node kinds gen_adjoint_body writes (fz_codegen.cpp); grad_unsupported_reason refuses a graph with any other
bool adjoint_takes(uint32_t kind);
// why the backward of a block does not support this graph ("" = it does): fz_grad.cpp
// rings_in_lds: float delay lines in LDS (depth 9 .. 256) are no objection -- the scope of fz_run_block_ring_grad
// rings_in_hbm (with rings_in_lds): float delay lines deeper than 256 samples are none either -- the scope of fz_run_block_far_grad
std::string grad_unsupported_reason(const Graph& g, bool rings_in_lds = false, bool rings_in_hbm = false);
// the far adjoint kernel's two static rules (fz_codegen.cpp, next to ring_layout, is their one home; include/flowz_hip.h states
// them).  A far read of sweep 1 is requested with its chunk's x rows when the row it reads was written before the chunk began; else
// it is a load of its own in front of its row.  Sweep 2 takes the fast path -- a chunk's pending adjoints requested together, added to in registers, stored
// once -- when no slot is touched twice within a chunk of C rows: every far read at least C rows old, any two of one line at least
// C apart; else the per-row path.
bool far_read_with_chunk(uint32_t delay, uint32_t C);
// the far states kernel's static rule (the same home): a far read travels with the next group's x rows when its delay is at least
// two groups of U rows -- the slot it reads was written before the request is issued; else it is a load of its own in front of its row
bool far_read_with_next_group(uint32_t delay, uint32_t U);
bool far_fast_path(const Graph& g, uint32_t C);
// could the backward have made this Variant of the adjoint family (FZ_VF_ADJOINT and the family bits next to it) for this graph?
// The flag set names the call; v fits when that call, asked for v's stride, makes exactly v: fz_grad.cpp
bool grad_variant_fits(const Graph& g, const Variant& v);
// 16-bit PCM frames (fz_pcm16.cpp): why the PCM kernel does not take this graph ("" = it does), and whether v is a Variant
// fz_run_block_pcm16 could have made for it
std::string pcm16_unsupported_reason(const Graph& g);
bool pcm16_variant_fits(const Graph& g, const Variant& v);
bool pcm16_sm_variant_fits(const Graph& g, const Variant& v);      // ... that fz_run_block_pcm16_stream_major could have made
// The forward of far lines on stream-major buffers (fz_far_sm.cpp): why fz_run_block_far_stream_major does not take this graph ("" =
// it does), and whether v is the Variant it makes for it
std::string far_sm_unsupported_reason(const Graph& g);
bool far_sm_variant_fits(const Graph& g, const Variant& v);

// ---- runtime ---------------------------------------------------------------------------------------------
// what the code object's metadata says the kernel needs (AMDGPU msgpack notes)
struct KernelResources {
   uint32_t vgprs = 0, agprs = 0, sgprs = 0;
   uint32_t scratch_bytes = 0;      // .private_segment_fixed_size: bytes of scratch memory per lane (register spills)
   uint32_t lds_bytes = 0;
   uint32_t vgpr_spills = 0, sgpr_spills = 0;
};

struct Kernel {
   std::mutex mu;                 // cache lookup / build / module loading of THIS variant (the program mutex is not held meanwhile)
   std::atomic<bool> built{false};
   KernelResources res;
   struct Loaded {
      int device;
      void* module;     // hipModule_t
      void* function;   // hipFunction_t
   };
   std::vector<char> code;        // code object (device independent: gfx950)
   std::string cache_path;        // on-disk cache file it came from / went to ("" = none)
   std::string code_id;           // 16 hex digits: hash of (source, options, the compiler that BUILT this object) = its file name in the cache
   std::vector<Loaded> loaded;    // one module per device the kernel ran on
   void* function_on_current_device(const std::string& symbol);   // loads on first use (caller holds `mu`)
   ~Kernel();                     // unloads the modules (fz_kernel_cache.cpp)
};

}  // namespace fz

namespace fz {
struct SideStream {        // hipStream_t / hipEvent_t, opaque here
   void* stream = nullptr;
   void* fork = nullptr;
   void* join = nullptr;
   std::unique_ptr<std::mutex> mu;   // held from the fork's record to the join's wait: the event pair belongs to one launch at a time
};
}  // namespace fz

struct fz_program {
   fz::Graph g;
   std::mutex mu;
   std::map<fz::Variant, std::shared_ptr<fz::Kernel>> kernels;
   // measured plans (fz_program_tune): (n_streams, tile_streams, device) -> the variant to use when the
   // caller passes none
   std::map<std::tuple<uint64_t, uint32_t, int>, fz_variant> plans;
   std::set<std::tuple<uint64_t, uint32_t, int>> tuned_default;   // shapes measured already (FLOWZ_HIP_AUTOTUNE)
   std::set<std::tuple<uint64_t, uint32_t, int>> measuring;       // shapes whose first big launch is measuring its plan right now (other launches of the shape wait)
   std::condition_variable measured;
   std::set<std::tuple<uint64_t, uint32_t, int>> plan_looked_up;  // shapes whose persisted plan (plans.txt of the kernel cache) was consulted
   std::string recipe;                                             // "typed <0|1> <input dtypes...>\n" + serialize_expr: how to compile this program again (kernel manifests); "" = not recorded
   uint64_t graph_hash = 0;                                        // structure of the lowered graph (no coefficient values)
   // FZ_VF_GRID_SYNC: arrival counters per device: 16 slices of `second` bytes, handed to the launches in turn (launches on
   // different streams may overlap and must not share counters; a slice comes round again after 15 other launches)
   std::map<int, std::pair<void*, size_t>> sync_dev;              // device -> (buffer, bytes per slice)
   std::vector<void*> sync_retired;                                // counter buffers that were outgrown: a captured hipGraph may still use them
   uint32_t sync_next = 0;
   std::map<int, fz::SideStream> side;                             // device -> side stream for remainder launches next to the laps (fz_launch.cpp)
   const float* mod_dev = nullptr;                                 // fz_program_set_modulation
   uint32_t mod_stride = 0;
   ~fz_program();                                                  // frees the counters (fz_launch.cpp)
};

namespace fz {
// what the caller asked for in a variant's flags (no variant: nothing)
inline bool uv_flag(const fz_variant* uv, uint32_t flag) { return uv && (uv->flags & flag); }
// the library's choice for a block shape; tile_streams 0 = plain time-major rows (stream-major frames: FZ_VF_STREAM_MAJOR in v->flags)
// allow_lockstep: the most streams per lane the CU-wide lockstep workgroups of plain time-major frames may use (0: not chosen at all)
Variant resolve_variant(const Graph& g, const fz_variant* v, uint64_t n_streams, uint32_t n_samples = 1u << 20, uint32_t tile_streams = 0,
                        uint32_t allow_lockstep = 4);
// plain time-major frames of many streams: streams per lane, lanes per workgroup, laps (one launch each), rows per chunk buffer, and
// the streams those laps cover (the rest: a remainder launch) -- fz_plan.cpp
struct TmGeometry {
   uint32_t P = 0, lanes = 0, laps = 0, U = 0;
   uint64_t main_streams = 0;
   double score = 0.0;
};
TmGeometry time_major_geometry(uint64_t n_streams, uint32_t max_p, bool heavy_ops, bool ragged_ok, uint32_t only_p = 0);
// planner rules that more than one file applies (fz_plan.cpp)
bool stage_pack_pays(const Graph& g, uint32_t n_samples);   // stage packing is automatic for blocks this long
bool heavy_ops(const Graph& g);                             // VALU-bound with one stream per lane (time_major_geometry's heavy_ops)
bool chunk_below_4gib(const Graph& g, uint64_t row_streams, bool out_f64, uint32_t U);   // U rows of the widest frame in one descriptor
bool sm_deep(const Graph& g);                              // stream-major: deep enough to be VALU-bound with one stream per lane
bool sm_long_stage_packs(const Graph& g);                   // the one-stream long-run body runs stage-packed by the library's choice
// the kernel a launch of that shape runs: resolved, fitted to the tile / the 4 GiB chunk limit, unroll lowered until nothing spills
Variant finalize_variant(fz_program* p, const fz_variant* v, uint64_t n_streams, uint32_t n_samples, uint32_t tile_streams, bool settle = true);
// what a launch runs: `main` over the streams [0, main_streams), and -- only when main_streams < n_streams -- `rem`, the remainder
// launch over the rest (lockstep laps of whole workgroups leave a few streams over)
struct LaunchPlan {
   Variant main;
   uint64_t main_streams = 0;
   Variant rem;
};
// rows_total: the rows of a stream-major buffer, 0 = not known (the pair body is not stepped down for long buffers);
// settle: as for finalize_variant; with_remainder = false: `rem` is not resolved (nothing is built for it)
LaunchPlan plan_launch(fz_program* p, const fz_variant* uv, uint64_t n_streams, uint32_t n_samples, uint32_t tile_streams, uint32_t rows_total = 0,
                       bool settle = true, bool with_remainder = true);
// builds (or fetches from the caches) the kernel of variant v; fn_out != null: also load it on the
// current device and return its hipFunction_t; build_in_own_process: a missing kernel is compiled by a process of its own (fz_rtc.cpp)
std::shared_ptr<Kernel> get_kernel(fz_program* p, const Variant& v, void** fn_out, bool build_in_own_process = false);
// what the kernel of variant v needs, as the inspection calls answer (builds or fetches it); `unroll` = v.U
inline fz_kernel_resources resources_of(fz_program* p, const Variant& v)
{
   const KernelResources r = get_kernel(p, v, nullptr)->res;
   return fz_kernel_resources{r.vgprs, r.agprs, r.sgprs, r.scratch_bytes, r.lds_bytes, r.vgpr_spills, r.sgpr_spills, v.U};
}
// the variant that runs: `v` with its unroll lowered until the kernel keeps its values in registers (no scratch memory): fz_plan.cpp
Variant settle_variant(fz_program* p, Variant v);
int launch(fz_program* p, const float* in, float* out, float* state, const float* params,
           uint64_t n_streams, uint32_t n_samples, const fz_variant* v, void* stream, uint32_t tile_streams = 0,
           uint32_t rows_total = 0, uint32_t row0 = 0, uint32_t mod_row0 = 0);   // mod_row0: row of the modulator arrays that goes with row 0 of the frame buffers
// fz_run_block_pcm16: argument checks, the static plan, the launch (fz_pcm16.cpp)
int launch_pcm16(fz_program* p, const void* in, void* out, float* state, const float* params, uint64_t n_streams, uint32_t n_samples,
                 uint32_t in_type, uint32_t out_type, void* stream);
// fz_run_block_pcm16_stream_major: the same for the window [row0, row0 + n_samples) of stream-major buffers
int launch_pcm16_sm(fz_program* p, const void* in, void* out, float* state, const float* params, uint64_t n_streams, uint32_t rows_total,
                    uint32_t row0, uint32_t n_samples, uint32_t in_type, uint32_t out_type, void* stream);
// fz_run_block_far_stream_major: the forward of a graph with far lines on the window of stream-major float32 buffers (fz_far_sm.cpp);
// a graph without a far line: fz_run_block_stream_major with a null variant
int launch_far_sm(fz_program* p, const float* in, float* out, float* state, const float* params, uint64_t n_streams, uint32_t rows_total,
                  uint32_t row0, uint32_t n_samples, void* stream);
int tune(fz_program* p, const float* in, float* out, float* state, const float* params, uint64_t n_streams,
         uint32_t n_samples, uint32_t tile_streams, void* stream, fz_variant* chosen, float* chosen_ms, bool implicit = false);
std::vector<fz_variant> tune_candidates(const Graph& g, uint64_t n_streams, uint32_t n_samples, uint32_t tile_streams);
// the plan a launch without a variant runs: measured by fz_program_tune (this process or, persisted, an earlier one), or -- with
// FLOWZ_HIP_AUTOTUNE=1 -- measured now by the first big launch of the shape on the caller's buffers; none: the library's static choice
std::optional<fz_variant> launch_plan_of_shape(fz_program* p, const float* in, float* out, float* state, const float* params, uint64_t n_streams,
                                               uint32_t n_samples, uint32_t tile_streams, uint32_t rows_total, uint32_t row0, void* stream);
int device_count();
uint64_t graph_structure_hash(const Graph& g);
// the plan a launch without a variant would use for this shape on the current device: in memory, else persisted, else {0,0,0,0}
fz_variant planned_variant(fz_program* p, uint64_t n_streams, uint32_t tile_streams);
void drop_plan(fz_program* p, uint64_t n_streams, uint32_t tile_streams);
// while one of these lives on a thread, get_kernel on that thread refuses to BUILD (FZ_E_UNSUPPORTED): cached objects only
extern thread_local bool tl_no_jit;
struct NoJitScope {
   bool before;
   explicit NoJitScope(bool on) : before(tl_no_jit) { tl_no_jit = on || before; }
   ~NoJitScope() { tl_no_jit = before; }
};
// is the kernel's code object at hand (in memory or in the on-disk cache), i.e. can it run without a hiprtc build?
bool kernel_at_hand(fz_program* p, const Variant& v);
std::string kernel_code_id(fz_program* p, const Variant& v);
int manifest_build(const std::string& path, unsigned n_workers, uint32_t counts[4]);   // fz_manifest.cpp

}  // namespace fz
