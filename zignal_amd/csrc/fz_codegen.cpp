// Lowered DAG -> the two generated headers the kernel skeleton includes.
//
// "fz_graph_config.h": sizes and variant knobs as macros.
// "fz_graph_body.h"  : struct fz_graph -- register delay lines / per-stream coefficients as
//                      members, and step(): the whole graph for one sample as straight-line code,
//                      one statement per DAG node in evaluation order (explicit temporaries, so the
//                      compiler cannot re-associate; contraction is disabled on the command line).
#include <algorithm>
#include <cstdio>
#include <functional>
#include <iterator>
#include <map>
#include <set>
#include <sstream>

#include "fz_internal.hpp"

namespace fz {

// fz_block_kernel.hip.inc and the kernel bodies, embedded at build time (embed.py)
extern const char* const kSkeletonHead;
extern const char* const kSkeletonBody_sm_common;    // what the three stream-major bodies share: in front of each of them
extern const char* const kSkeletonBody_sm_pair;
extern const char* const kSkeletonBody_sm_long;
extern const char* const kSkeletonBody_sm_short;
extern const char* const kSkeletonBody_wave_split;
extern const char* const kSkeletonBody_frames;
extern const char* const kSkeletonAdjoint;       // fz_kernel_adjoint.hip.inc: a kernel text of its own, like the five below
extern const char* const kSkeletonAdjointSm;
extern const char* const kSkeletonAdjointRing;   // fz_kernel_adjoint_ring.hip.inc: rings in LDS and, with FZ_FAR, delay lines deeper than 256 samples, rings in HBM
extern const char* const kSkeletonAdjointRingSm; // fz_kernel_adjoint_ring_sm.hip.inc: the same on stream-major buffers
extern const char* const kSkeletonStates;        // fz_kernel_states.hip.inc: plain, with FZ_RING ring, and with FZ_FAR next to it far
extern const char* const kSkeletonStatesSm;      // fz_kernel_states_sm.hip.inc: the same three modes on stream-major buffers
extern const char* const kSkeletonPcm16;     // fz_kernel_pcm16.hip.inc: the frame walk for 16-bit PCM frames, behind the common head
extern const char* const kSkeletonPcm16Sm;   // fz_kernel_pcm16_sm.hip.inc: the same for stream-major buffers
extern const char* const kSkeletonFarSm;     // fz_kernel_far_sm.hip.inc: the forward of far lines on stream-major buffers, behind the common head

// The adjoint family (fz_grad.cpp), layout x rings plus the states kernels: one row per combination of the family bits next to
// FZ_VF_ADJOINT, found by exact match: a row per symbol stem.  The loss selects no row: it is FZ_LOSS in the configuration of the row's
// text and "_loss" in the symbol, fz_<head>[_loss]<tail>_kernel_<c|u><U>[r<P>]b<block>.  The states rows' text is chosen by the layout
// alone: the ring is FZ_RING in its configuration.  Neither do the rings in HBM select a text: a far row has its ring sibling's, with
// FZ_FAR 1 in its configuration.
struct AdjointRow {
   uint32_t bits;               // of FZ_VF_STATES | FZ_VF_ADJOINT_RING | FZ_VF_ADJOINT_SM | FZ_VF_ADJOINT_FAR
   const char *head, *tail;     // of the symbol's stem
   std::string text;            // the hand-written kernel
   bool patch_rows;             // the symbol carries r<P>: the rows of the LDS patch of the stream-major frames
};
static const AdjointRow& adjoint_row(const Variant& v)
{
   static const AdjointRow rows[] = {
      {0, "fz_adjoint", "", kSkeletonAdjoint, false},
      {FZ_VF_ADJOINT_SM, "fz_adjoint", "_sm", kSkeletonAdjointSm, true},
      {FZ_VF_ADJOINT_RING, "fz_adjoint_ring", "", kSkeletonAdjointRing, false},
      {FZ_VF_ADJOINT_RING | FZ_VF_ADJOINT_SM, "fz_adjoint_ring", "_sm", kSkeletonAdjointRingSm, true},
      {FZ_VF_ADJOINT_RING | FZ_VF_ADJOINT_FAR, "fz_adjoint_far", "", kSkeletonAdjointRing, false},
      {FZ_VF_ADJOINT_RING | FZ_VF_ADJOINT_FAR | FZ_VF_ADJOINT_SM, "fz_adjoint_far", "_sm", kSkeletonAdjointRingSm, true},
      {FZ_VF_STATES, "fz_states", "", kSkeletonStates, false},
      {FZ_VF_STATES | FZ_VF_ADJOINT_SM, "fz_states", "_sm", kSkeletonStatesSm, true},
      {FZ_VF_STATES | FZ_VF_ADJOINT_RING, "fz_states", "_ring", kSkeletonStates, false},
      {FZ_VF_STATES | FZ_VF_ADJOINT_RING | FZ_VF_ADJOINT_SM, "fz_states", "_ring_sm", kSkeletonStatesSm, true},
      {FZ_VF_STATES | FZ_VF_ADJOINT_RING | FZ_VF_ADJOINT_FAR, "fz_states", "_far", kSkeletonStates, false},
      {FZ_VF_STATES | FZ_VF_ADJOINT_RING | FZ_VF_ADJOINT_FAR | FZ_VF_ADJOINT_SM, "fz_states", "_far_sm", kSkeletonStatesSm, true},
   };
   for (const AdjointRow& r : rows)
      if (r.bits == (v.flags & (FZ_VF_STATES | FZ_VF_ADJOINT_RING | FZ_VF_ADJOINT_SM | FZ_VF_ADJOINT_FAR)) && !((v.flags & FZ_VF_STATES) && (v.flags & FZ_VF_ADJOINT_LOSS))) return r;
   fail(FZ_E_INVALID, "internal: no kernel of the adjoint family has the flags " + std::to_string(v.flags));
}

// the hand-written text of a variant's kernel: the common head + the ONE body its flags (stream-major: and its streams per lane) select
const std::string& skeleton_source(const Variant& v)
{
   static const std::string head = kSkeletonHead, sm = head + kSkeletonBody_sm_common;
   static const std::string sm_pair = sm + kSkeletonBody_sm_pair, sm_long = sm + kSkeletonBody_sm_long, sm_short = sm + kSkeletonBody_sm_short,
                            ws = head + kSkeletonBody_wave_split, fr = head + kSkeletonBody_frames;
   static const std::string pcm = head + kSkeletonPcm16, pcm_sm = head + kSkeletonPcm16Sm, far_sm = head + kSkeletonFarSm;
   if (v.flags & FZ_VF_ADJOINT) return adjoint_row(v).text;
   if (v.flags & FZ_VF_PCM16) return (v.flags & FZ_VF_PCM16_SM) ? pcm_sm : pcm;
   if (is_far_sm(v.flags)) return far_sm;
   if (v.flags & FZ_VF_STREAM_MAJOR) return !(v.flags & FZ_VF_SM_LONG) ? sm_short : v.P == 2 ? sm_pair : sm_long;
   return ws_parts(v.flags) ? ws : fr;
}

// one symbol per variant, so that profilers (rocprofv3 --stats) keep the variants apart:
// fz_block_kernel_p<streams/lane>u<unroll>b<block>[s<segments>]f<flags>
std::string kernel_name(const Graph& g, const Variant& v)
{
   if (v.flags & FZ_VF_ADJOINT) {   // (the family bits mean something next to FZ_VF_ADJOINT only)
      const AdjointRow& r = adjoint_row(v);
      return std::string(r.head) + ((v.flags & FZ_VF_ADJOINT_LOSS) ? "_loss" : "") + r.tail + "_kernel_" + ((v.flags & FZ_VF_STATES) ? "u" : "c") + std::to_string(v.U) +
             (r.patch_rows ? "r" + std::to_string(v.P) : "") + "b" + std::to_string(v.block);
   }
   if ((v.flags & FZ_VF_PCM16) && (v.flags & FZ_VF_PCM16_SM))   // (stream-major PCM: which side is int16, rows per chunk, lanes)
      return "fz_pcm16_sm_kernel_i" + std::to_string((v.flags & FZ_VF_PCM16_IN) ? 1 : 0) + "o" + std::to_string((v.flags & FZ_VF_PCM16_OUT) ? 1 : 0) + "u" +
             std::to_string(v.U) + "b" + std::to_string(v.block);
   // (PCM frames: which side is int16, then h = 2-byte accesses -- int16 rows off the dword grid --, m = merging stores)
   if (v.flags & FZ_VF_PCM16)
      return "fz_pcm16_kernel_i" + std::to_string((v.flags & FZ_VF_PCM16_IN) ? 1 : 0) + "o" + std::to_string((v.flags & FZ_VF_PCM16_OUT) ? 1 : 0) + "p" +
             std::to_string(v.P) + "u" + std::to_string(v.U) + "b" + std::to_string(v.block) + ((v.flags & FZ_VF_PCM16_B16) ? "h" : "") +
             ((v.flags & FZ_VF_ST_MERGE) ? "m" : "");
   // (the forward of far lines on stream-major buffers: rows of an unrolled group, rows of the patch, lanes)
   if (is_far_sm(v.flags)) return "fz_far_sm_kernel_g" + std::to_string(v.U) + "r" + std::to_string(v.P) + "b" + std::to_string(v.block);
   std::string n = "fz_block_kernel_p" + std::to_string(v.P) + "u" + std::to_string(v.U) + "b" + std::to_string(v.block);
   if ((v.flags & FZ_VF_STAGE_PACK) && g.split.ok) n += "s" + std::to_string(g.split.K) + (g.split.m > 1 ? "a" + std::to_string(g.split.m) : "");
   if (ws_parts(v.flags)) n += "w" + std::to_string(ws_parts(v.flags)) + (ws_io(v.flags) ? (ws_io_waves(v.flags) == 2 ? "io2" : "io") : "");
   // (the flags the caller can set, then one letter per INTERNAL bit the launch path added: R rows clipped per descriptor (a count that is
   //  not a multiple of the streams per lane), M merging stores (rows off the 64-byte grid), L the lane's four streams as
   //  two pairs 128 apart, S the lane's streams 64 apart)
   constexpr uint32_t internal = FZ_VF_RAGGED | FZ_VF_ST_MERGE | FZ_VF_LANE_PAIRS | FZ_VF_LANE_SINGLES;
   return n + "f" + std::to_string(v.flags & ~internal) + ((v.flags & FZ_VF_RAGGED) ? "R" : "") + ((v.flags & FZ_VF_ST_MERGE) ? "M" : "") +
          ((v.flags & FZ_VF_LANE_PAIRS) ? "L" : "") + ((v.flags & FZ_VF_LANE_SINGLES) ? "S" : "");
}

// The symbol a profiler sees: the variant AND the graph -- two graphs that run the same variant (the 6-biquad cascade and a single
// biquad both take four streams per lane in 1024-lane workgroups) must not share a row of `rocprofv3 --stats` (round 4: the average
// over "fz_block_kernel_p4u1b1024f8912928" mixed a dozen workloads of the bench line).  The tag is the graph's STRUCTURE (no
// coefficient values: graphs that differ in literals only share code objects and symbols).
std::string kernel_symbol(const Graph& g, const Variant& v)
{
   char tag[16];
   std::snprintf(tag, sizeof tag, "_g%08x", g.sym_tag);
   return kernel_name(g, v) + tag;
}

// LDS rings of the frame kernels, VECTORISED IN TIME (round 5).  Round 4 kept a ring as `ring[slot][lane]`: one ds_read and one
// ds_write of a lane's 4 P bytes per line and step, and a read younger than the chunk (the 23-sample comb under 32-row chunks) was
// issued where it was needed -- one LDS round trip per step with one or two waves per SIMD to hide it behind.  Now a lane's slots
// are CONTIGUOUS (`ring[line][lane][slot][stream of the lane]`, rows padded by 16 bytes: the lanes of every 16-byte access group fall on
// distinct banks), the chunk runs in SUB-CHUNKS of G steps (G = the largest power of two <= the youngest ring read, <= the chunk): all
// ring reads of a sub-chunk refer to slots written before it began and are fetched together as 16-byte vectors (4 / P time steps each),
// and its pushes are kept in registers and written as 16-byte vectors when it ends.  A read `d` samples back starts (-d) mod (4 / P)
// slots off the 16-byte grid -- a constant: the aligned vectors around it are read and the step's value is a register of them.
RingPlan ring_plan(const Graph& g, const Variant& v)
{
   RingPlan rp;
   rp.slots = g.n_lds_slots;
   if (!g.n_lds_slots || (v.flags & (FZ_VF_STREAM_MAJOR | FZ_VF_STAGE_PACK)) || is_far_sm(v.flags) || ws_parts(v.flags) || v.P > 4 || v.U < 2) return rp;
   const uint32_t TW = 4 / v.P;
   uint32_t min_read = ~0u;
   std::set<std::pair<uint32_t, uint32_t>> reads;
   for (const Node& nd : g.nodes) {
      if (nd.kind != FZ_IR_DELAY) continue;
      const Line& L = g.lines[(size_t)g.line_of_node[nd.a]];
      if (!L.in_lds) continue;
      if (L.f64) return rp;                                  // (double rings: two word planes, read in place)
      min_read = std::min(min_read, nd.b);
      reads.insert({(uint32_t)g.line_of_node[nd.a], nd.b});
   }
   uint32_t n_lines = 0;
   for (const Line& L : g.lines)
      if (L.in_lds) {
         if (L.f64 || (L.lds_size & (L.lds_size - 1)) || L.lds_size % TW) return rp;
         ++n_lines;
      }
   if (min_read == ~0u) min_read = v.U;                      // (lines nobody reads from LDS: pushes only)
   uint32_t G = 1;
   while (G * 2 <= min_read && G * 2 <= v.U) G *= 2;
   while (G > 1 && v.U % G) G /= 2;
   auto regs = [&](uint32_t gg) {
      uint32_t r = n_lines * gg * v.P;
      for (const auto& rd : reads) r += ((((TW - rd.second % TW) % TW) + gg + TW - 1) / TW) * 4;
      return r;
   };
   while (G > TW && regs(G) > 200) G /= 2;
   if (G < TW || G < 2 || regs(G) > 200) return rp;
   rp.vec = true;
   rp.G = G;
   rp.TW = TW;
   rp.pad = 4 / v.P;
   uint32_t lane = 0;
   for (const Line& L : g.lines)
      if (L.in_lds) lane += (L.lds_size + rp.pad) * v.P;
   rp.lane_floats = lane;
   rp.slots = (lane + v.P - 1) / v.P;
   return rp;
}

// LDS ring reads of a chunk, fetched TOGETHER at the start of the chunk (round 4).  A read `n - d` inside step() cannot be moved
// above the ring write of the step before it (the compiler cannot tell the slots apart), so every step waited one LDS round trip per
// line with nothing to hide it behind (one or two waves per SIMD: the rings fill the LDS) -- 240 clocks per step for the two combs of
// the bench line's lds_ring graph.  A read whose delay is at least the chunk length refers to a slot written BEFORE the chunk
// started, for every step of the chunk: all of a chunk's reads can be issued up front, into registers (`lr<k>[u]`), one round
// trip per chunk.  Float lines, frame kernels (the stream-major bodies call step() without a chunk position and read in place);
// at most 96 registers.  Vectorised rings (ring_plan) fetch every read of a sub-chunk this way.
struct RingRead { uint32_t line, d, m, nv; };              // m: slots between the 16-byte grid and the read's first slot; nv: vectors per sub-chunk
static std::vector<RingRead> ring_reads(const Graph& g, const Variant& v, const RingPlan& rp)
{
   std::vector<RingRead> r;
   if (!rp.vec && ((v.flags & FZ_VF_STREAM_MAJOR) || is_far_sm(v.flags) || v.U < 2)) return r;
   for (const Node& nd : g.nodes) {
      if (nd.kind != FZ_IR_DELAY) continue;
      const uint32_t l = (uint32_t)g.line_of_node[nd.a];
      const Line& L = g.lines[l];
      if (!L.in_lds || (!rp.vec && (L.f64 || L.far || nd.b < v.U))) continue;
      if (std::any_of(r.begin(), r.end(), [&](const RingRead& x) { return x.line == l && x.d == nd.b; })) continue;
      const uint32_t m = rp.vec ? (rp.TW - nd.b % rp.TW) % rp.TW : 0;
      r.push_back(RingRead{l, nd.b, m, rp.vec ? (m + rp.G + rp.TW - 1) / rp.TW : 0});
   }
   if (!rp.vec && r.size() * v.U * v.P > 96) r.clear();
   return r;
}

std::string gen_config(const Graph& g, const Variant& v)
{
   if (v.flags & FZ_VF_ADJOINT) return gen_adjoint_config(g, v);
   std::ostringstream o;
   o << "// generated by libflowz_hip -- graph configuration\n";
   o << "#define FZ_NIN " << g.n_in << "\n";
   o << "#define FZ_NOUT " << g.n_out << "\n";
   o << "#define FZ_NCONST " << g.consts.size() << "\n";
   o << "#define FZ_NCONST64 " << g.consts64.size() << "\n";
   o << "#define FZ_NPARAM " << g.n_param << "\n";
   o << "#define FZ_NMOD " << g.n_mod << "\n";
   o << "#define FZ_NSTATE " << g.n_state << "\n";
   // (the far stream-major forward carries its patch rows in P: FZ_R; the body is compiled for one stream per lane)
   o << "#define FZ_P " << (is_far_sm(v.flags) ? 1u : v.P) << "\n";
   if (is_far_sm(v.flags)) o << "#define FZ_R " << v.P << "\n";
   o << "#define FZ_U " << v.U << "\n";
   o << "#define FZ_BLOCK " << v.block << "\n";
   o << "#define FZ_FLAGS " << v.flags << "u\n";
   const RingPlan rp = ring_plan(g, v);
   o << "#define FZ_LDS_SLOTS " << rp.slots << "   // V slots per lane of the LDS rings\n";
   o << "#define FZ_RING_G " << (rp.vec ? rp.G : 0u) << "   // LDS rings vectorised in time: reads fetched / pushes flushed every so many steps (0: in place)\n";
   // the long-run stream-major body with 64-sample phases: patches of 19 KB per wave, so two workgroups fit a CU -- if the
   // kernel stays within 256 registers (it needs 258 left alone): ask for two waves per SIMD
   o << "#define FZ_MINWAVES " << (((v.flags & FZ_VF_SM_LONG) && v.U == 64 && v.P == 1) ? 2 : 0) << "\n";
   {  // occupancy cap (flags bits 20..22 = max workgroups per CU): pad the workgroup's LDS so that no
      // more than that many fit into the CU's 160 KiB
      const uint32_t cap = (v.flags >> 20) & 7u;
      uint32_t pad = 0;
      if (cap) {
         const uint32_t ring = rp.slots * v.block * 4u * v.P, want = 160u * 1024u / (cap + 1) + 1024u;
         pad = want > ring ? (std::min(want, 160u * 1024u) - ring) / 4u : 0u;
      }
      o << "#define FZ_OCC_PAD " << pad << "\n";
   }
   o << "#define FZ_KERNEL " << kernel_symbol(g, v) << "\n";
   o << "#define FZ_NFR " << g.far_reads.size() << "   // far (HBM ring) delayed reads per sample\n";
   o << "#define FZ_NFW " << g.far_lines.size() << "   // far delay lines = ring rows written per sample\n";
   // FZ_SKEW = lag of the last segment behind the first one (number of segments - 1), 0 = off
   o << "#define FZ_SKEW " << ((v.flags & FZ_VF_STAGE_PACK) && g.split.ok ? g.split.atoms() - 1 : 0) << "\n";
   if (const uint32_t W = ws_parts(v.flags)) {
      const std::vector<Graph>* roles = g.wave_roles(W);
      if (!roles) fail(FZ_E_UNSUPPORTED, "wave split: the graph is not that many isomorphic parts in series");
      o << "#define FZ_WS_W " << W << "   // compute waves per stream tuple = parts of the graph\n";
      o << "#define FZ_WS_IO " << ws_io(v.flags) << "   // one more wave per tuple for the frame I/O\n";
      o << "#define FZ_WS_IOW " << ws_io_waves(v.flags) << "   // ... or two: a loader and a storer\n";
      for (uint32_t k = 0; k < 4; ++k)
         o << "#define FZ_WS_K" << k << " " << (k < W && roles ? (*roles)[k].split.atoms() : 0u) << "   // skewed units (segments x atoms) of part " << k << "\n";
   }
   return o.str();
}

// How every operation kind is written in C++, for all the generated bodies.  `op`: the operator where C++ has one; `fn`: the device
// function the text calls.  Division and the comparisons have both: the frame body calls fz_div / fz_cmp<K> on a lane's streams, the
// scalar bodies (stage packing, the adjoint) use the operator -- a comparison as (a < b) ? 1.f : 0.f.
struct OpSpelling { uint32_t kind; const char* op; const char* fn; uint32_t arity; };
static const OpSpelling kOps[] = {
   {FZ_IR_ADD, "+", nullptr, 2}, {FZ_IR_SUB, "-", nullptr, 2}, {FZ_IR_MUL, "*", nullptr, 2}, {FZ_IR_DIV, "/", "fz_div", 2},
   {FZ_IR_NEG, "-", nullptr, 1}, {FZ_IR_WIDEN, nullptr, "fz_cvt_d", 1}, {FZ_IR_NARROW, nullptr, "fz_cvt_f", 1},
   {FZ_IR_ABSLT, nullptr, "fz_abs_lt", 2}, {FZ_IR_SELECT, nullptr, "fz_select", 3},
   {FZ_IR_LT, "<", "fz_cmp", 2}, {FZ_IR_LE, "<=", "fz_cmp", 2}, {FZ_IR_GT, ">", "fz_cmp", 2}, {FZ_IR_GE, ">=", "fz_cmp", 2},
   {FZ_IR_EQ, "==", "fz_cmp", 2}, {FZ_IR_NE, "!=", "fz_cmp", 2},
   {FZ_IR_ABS, nullptr, "fz_abs", 1}, {FZ_IR_SQRT, nullptr, "fz_sqrt", 1}, {FZ_IR_EXP, nullptr, "fz_exp", 1}, {FZ_IR_TANH, nullptr, "fz_tanh", 1},
   {FZ_IR_MIN, nullptr, "fz_min", 2}, {FZ_IR_MAX, nullptr, "fz_max", 2},
   {FZ_IR_SIN, nullptr, "fz_sin", 1}, {FZ_IR_COS, nullptr, "fz_cos", 1}, {FZ_IR_LOG, nullptr, "fz_log", 1},
};

// the graph functions are the kinds FZ_IR_ABS .. FZ_IR_LOG (FZ_IR_MAX is std::max, not the last of them)
static constexpr uint32_t kFnFirst = FZ_IR_ABS, kFnLast = FZ_IR_LOG;

static bool is_cmp(uint32_t kind) { return kind >= FZ_IR_LT && kind <= FZ_IR_NE; }

// operand k (0: a, 1: b, 2: c) of a node
static uint32_t operand(const Node& nd, uint32_t k) { return k == 0 ? nd.a : k == 1 ? nd.b : nd.c; }

// The right-hand side of an operation node, "" for any other kind (inputs, coefficients, delayed reads: each body reads those from
// where it keeps them).  x(k, common) writes operand k as the body names it; common: the operand is taken in the operation's common
// type (every operand of a binary operation, the two sides of a selection), which the frame body reaches by promoting float to double.
// frame: the frame body's spelling, else the scalar bodies'.
static std::string op_expr(uint32_t kind, bool frame, const std::function<std::string(uint32_t, bool)>& x)
{
   const OpSpelling* s = std::find_if(std::begin(kOps), std::end(kOps), [&](const OpSpelling& t) { return t.kind == kind; });
   if (s == std::end(kOps)) return "";
   if (s->op && !(frame && s->fn)) {
      if (s->arity == 1) return s->op + x(0, false);
      const std::string e = x(0, true) + " " + s->op + " " + x(1, true);
      return is_cmp(kind) ? "(" + e + ") ? 1.f : 0.f" : e;
   }
   std::string e = std::string(s->fn) + (is_cmp(kind) ? "<" + std::to_string(kind) + ">" : "") + "(";
   for (uint32_t k = 0; k < s->arity; ++k) e += (k ? ", " : "") + x(k, s->arity > 1 && !(kind == FZ_IR_SELECT && k == 0));
   return e + ")";
}

// One step of a delay line kept in registers: age a takes age a - 1 (a = depth .. 2), age 1 takes the new value `in`; reg(a) names the
// register of age a.  With a guard (the masked steps of a stage-packed body: does the line's segment run?) a register keeps its value
// where the guard is false; a packed pair of lines has a guard per half (guard: .x, guard_y: .y).
static void shift_line(std::ostringstream& o, uint32_t depth, const std::function<std::string(uint32_t)>& reg, const std::string& in,
                       const std::string& guard = "", const std::string& guard_y = "")
{
   for (uint32_t a = depth; a >= 1; --a) {
      const std::string r = reg(a), nv = a == 1 ? in : reg(a - 1);
      o << "      " << r << " = ";
      if (guard.empty()) o << nv;
      else if (guard_y.empty()) o << guard << " ? " << nv << " : " << r;
      else o << "(fz_f2){" << guard << " ? " << nv << ".x : " << r << ".x, " << guard_y << " ? " << nv << ".y : " << r << ".y}";
      o << ";\n";
   }
}

static std::string gen_body_skew(const Graph& g, const StageSplit& sp);

// The graph functions (FZ_IR_ABS .. FZ_IR_LOG) for V and VD, written only into the text of graphs that use them: every other graph keeps
// its kernel source byte for byte.  Branch-free per lane (both sides computed, the lane's one selected); exp and tanh are IEEE +, -, *,
// correctly rounded / and exact power-of-two scaling through the exponent bits, no FMA (-ffp-contract=off), no hardware approximation and
// no library call -- tests/fn_ref.py restates them operation for operation.  The polynomials run on V / VD themselves, so that two or four
// streams per lane issue packed v_pk_mul_f32 / v_pk_add_f32; the comparisons and the exponent bits are per element (vector ternaries).
// adjoint: the text is for an adjoint kernel, whose rules for sin and cos call the other one of the two on the operand.
static void emit_functions(std::ostringstream& o, const Graph& g, bool adjoint = false)
{
   bool has[kFnLast + 1] = {};
   for (const Node& nd : g.nodes)
      if (nd.kind >= kFnFirst && nd.kind <= kFnLast) has[nd.kind] = true;
   if (has[FZ_IR_TANH]) has[FZ_IR_EXP] = true;
   if (adjoint && (has[FZ_IR_SIN] || has[FZ_IR_COS])) has[FZ_IR_SIN] = has[FZ_IR_COS] = true;
   bool any = false;
   for (uint32_t k = kFnFirst; k <= kFnLast; ++k) any = any || has[k];
   if (!any) return;
   o << "#if FZ_P == 1\ntypedef int fz_vi;\ntypedef long long fz_vl;\n#else\n"
        "typedef int fz_vi __attribute__((ext_vector_type(FZ_P)));\ntypedef long long fz_vl __attribute__((ext_vector_type(FZ_P)));\n#endif\n";
   if (has[FZ_IR_SIN] || has[FZ_IR_COS] || has[FZ_IR_LOG])   // value conversions per element (a C cast of a vector would be a bit cast)
      o << "#if FZ_P == 1\n#define FZ_CVT(x, T) ((T)(x))\n#else\n#define FZ_CVT(x, T) __builtin_convertvector(x, T)\n#endif\n";
   if (has[FZ_IR_SIN] || has[FZ_IR_COS]) {
      // std::sin / std::cos of a float: the algorithm and the constants of fz_sincos_f32 (fz_aot_kernels.hip), restated for the streams of
      // a lane; the double-precision core is shared by the two functions
      static const char* const ps[] = {"0x1.952c77030ad4ap-49", "-0x1.ae7f3e733b81fp-41", "0x1.6124613a86d09p-33", "-0x1.ae64567f544e4p-26",
                                       "0x1.71de3a556c734p-19", "-0x1.a01a01a01a01ap-13", "0x1.1111111111111p-7", "-0x1.5555555555555p-3"};
      static const char* const pc[] = {"-0x1.6827863b97d97p-53", "0x1.ae7f3e733b81fp-45", "-0x1.93974a8c07c9dp-37", "0x1.1eed8eff8d898p-29", "-0x1.27e4fb7789f5cp-22",
                                       "0x1.a01a01a01a01ap-16", "-0x1.6c16c16c16c17p-10", "0x1.5555555555555p-5", "-0x1.0000000000000p-1"};
      o << "// s = sin r, c = cos r and the quadrant q = k & 3 of a = k pi/2 + r, in double; ok: |a| < 2^20 (else the core runs on 0)\n";
      o << "__device__ __forceinline__ void fz_sincos_core(V a, VD& s, VD& c, fz_vl& q, fz_vi& ok)\n{\n";
      o << "   ok = (__builtin_bit_cast(fz_vi, a) & (fz_vi)(0x7fffffff)) < (fz_vi)(0x49800000);   // |a| < 2^20; false for inf and NaN\n";
      o << "   const V af = ok ? a : (V)(0);\n";
      o << "   const VD x = FZ_CVT(af, VD);\n";
      o << "   const VD t = x * (VD)(0x1.45f306dc9c883p-1);   // x * 2/pi\n";
      o << "   const VD th = t + (t < (VD)(0) ? (VD)(-0.5) : (VD)(0.5));\n";
      o << "   const fz_vi k = FZ_CVT(th, fz_vi);   // nearest integer (the conversion truncates)\n";
      o << "   const VD kd = FZ_CVT(k, VD);\n";
      o << "   VD r = x - kd * (VD)(0x1.921fb54400000p+0);   // pi/2, first 33 bits: the product is exact\n";
      o << "   r = r - kd * (VD)(0x1.0b4611a600000p-34);\n";
      o << "   r = r - kd * (VD)(0x1.3198a2e037073p-69);\n";
      o << "   const VD z = r * r;\n";
      o << "   VD ps = (VD)(" << ps[0] << ");\n";
      for (size_t k = 1; k < std::size(ps); ++k) o << "   ps = (VD)(" << ps[k] << ") + z * ps;\n";
      o << "   s = r + r * (z * ps);\n";
      o << "   VD pc = (VD)(" << pc[0] << ");\n";
      for (size_t k = 1; k < std::size(pc); ++k) o << "   pc = (VD)(" << pc[k] << ") + z * pc;\n";
      o << "   c = (VD)(1) + z * pc;\n";
      o << "   q = FZ_CVT(k, fz_vl) & (fz_vl)(3);\n}\n";
      for (int cosine = 0; cosine < 2; ++cosine) {
         if (!has[cosine ? FZ_IR_COS : FZ_IR_SIN]) continue;
         o << "__device__ __forceinline__ V " << (cosine ? "fz_cos" : "fz_sin") << "(V a)\n{\n";
         o << "   // quadrant 0..3: " << (cosine ? "c, -s, -c, s" : "s, c, -s, -c") << "; one rounding to float; |a| >= 2^20, inf, NaN: NaN\n";
         o << "   VD s, c;\n   fz_vl q;\n   fz_vi ok;\n   fz_sincos_core(a, s, c, q, ok);\n";
         o << "   const VD m = (q & (fz_vl)(1)) != (fz_vl)(0) ? " << (cosine ? "s : c" : "c : s") << ";\n";
         o << "   const VD y = (" << (cosine ? "(q + (fz_vl)(1))" : "q") << " & (fz_vl)(2)) != (fz_vl)(0) ? -m : m;\n";
         o << "   " << (cosine ? "const V yf = FZ_CVT(y, V);\n" : "V yf = FZ_CVT(y, V);\n   yf = a == (V)(0) ? a : yf;   // sin(+-0) = +-0 (r + r (z S) is +0 for r = -0)\n");
         o << "   return ok ? yf : (V)(__builtin_nanf(\"\"));\n}\n";
      }
   }
   struct Ty {
      const char *T, *I, *sfx, *magic, *log2e, *ln2hi, *ln2lo, *xlo, *xhi, *xmax, *sw, *sat, *sign, *bias;
      int shift;
      std::vector<const char*> q, p;
   };
   const Ty tys[2] = {
      {"V", "fz_vi", "f", "0x1.8p+23f", "0x1.715476p+0f", "0x1.62ep-1f", "0x1.0bfbe8p-15f", "-104.0f", "89.0f", "0x1.62e42ep+6f",
       "0x1.19999ap-1f", "10.0f", "(fz_vi)(-2147483647 - 1)", "127", 23,
       {"0x1.a127fcp-13f", "0x1.6d469p-10f", "0x1.1110ep-7f", "0x1.5554e6p-5f", "0x1.555556p-3f", "0x1p-1f"},
       {"0x1.4b0ed2p-9f", "-0x1.176084p-7f", "0x1.6578cap-6f", "-0x1.ba1428p-5f", "0x1.111104p-3f", "-0x1.555556p-2f"}},
      {"VD", "fz_vl", "", "0x1.8p+52", "0x1.71547652b82fep+0", "0x1.62e42fee00000p-1", "0x1.a39ef35793c76p-33", "-746.0", "710.0",
       "0x1.62e42fefa39efp+9", "0x1.19999ap-1", "20.0", "(fz_vl)(-9223372036854775807LL - 1)", "1023", 52,
       {"0x1.1f74882ae4b27p-29", "0x1.af509232e2477p-26", "0x1.27e4daa87b888p-22", "0x1.71de00e89dd34p-19", "0x1.a01a01a714245p-16",
        "0x1.a01a01ac50533p-13", "0x1.6c16c16c16266p-10", "0x1.111111111001cp-7", "0x1.5555555555556p-5", "0x1.5555555555557p-3", "0x1p-1"},
       {"0x1.081656de10f02p-17", "-0x1.1ad1adfc0e63cp-15", "0x1.8c8f32860a20fp-14", "-0x1.f41c32178e2b0p-13", "0x1.3547b24884a3fp-11",
        "-0x1.7da25c9e6e474p-10", "0x1.d6d3c5f32768dp-9", "-0x1.226e353986e33p-7", "0x1.664f48822db68p-6", "-0x1.ba1ba1ba1a711p-5",
        "0x1.1111111111109p-3", "-0x1.5555555555555p-2"}},
   };
   for (const Ty& t : tys) {
      const std::string T = t.T, I = t.I, c = "(" + T + ")";
      auto head = [&](const char* name, bool two) {
         o << "__device__ __forceinline__ " << T << " " << name << "(" << T << " a" << (two ? ", " + T + " b" : std::string()) << ")\n{\n";
      };
      if (has[FZ_IR_ABS]) {
         head("fz_abs", false);
         o << "   return __builtin_bit_cast(" << T << ", __builtin_bit_cast(" << I << ", a) & ~" << t.sign << ");   // std::fabs: clear the sign bit\n}\n";
      }
      if (has[FZ_IR_SQRT]) {   // correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt; the double expansion is exact too)
         head("fz_sqrt", false);
         o << "#if FZ_P == 1\n   return __builtin_sqrt" << t.sfx << "(a);\n#else\n   " << T << " r;\n#pragma unroll\n   for (int j = 0; j < FZ_P; ++j) r[j] = __builtin_sqrt"
           << t.sfx << "(a[j]);\n   return r;\n#endif\n}\n";
      }
      if (has[FZ_IR_MIN]) {
         head("fz_min", true);
         o << "   return (b < a) ? b : a;   // std::min\n}\n";
      }
      if (has[FZ_IR_MAX]) {
         head("fz_max", true);
         o << "   return (a < b) ? b : a;   // std::max\n}\n";
      }
      if (has[FZ_IR_EXP]) {
         head("fz_exp", false);
         o << "   // k = rint(a / ln 2) by the 1.5 * 2^(p-1) trick, r = (a - k ln2_hi) - k ln2_lo (k ln2_hi exact), e^r = 1 + (r + r^2 q(r)),\n"
              "   // then * 2^(k >> 1) (exact) * 2^(k - (k >> 1)) (one rounding, also into the subnormals)\n";
         o << "   " << T << " x = a < " << c << "(" << t.xlo << ") ? " << c << "(" << t.xlo << ") : a;\n";
         o << "   x = x > " << c << "(" << t.xhi << ") ? " << c << "(" << t.xhi << ") : x;\n";
         o << "   x = x == x ? x : " << c << "(0);\n";
         o << "   const " << T << " tm = x * " << c << "(" << t.log2e << ") + " << c << "(" << t.magic << ");\n";
         o << "   const " << T << " kf = tm - " << c << "(" << t.magic << ");\n";
         o << "   const " << T << " r = (x - kf * " << c << "(" << t.ln2hi << ")) - kf * " << c << "(" << t.ln2lo << ");\n";
         o << "   " << T << " q = " << c << "(" << t.q[0] << ");\n";
         for (size_t k = 1; k < t.q.size(); ++k) o << "   q = " << c << "(" << t.q[k] << ") + r * q;\n";
         o << "   const " << T << " p = " << c << "(1) + (r + (r * r) * q);\n";
         o << "   const " << I << " k = __builtin_bit_cast(" << I << ", tm) - __builtin_bit_cast(" << I << ", " << c << "(" << t.magic << "));\n";
         o << "   const " << I << " k1 = k >> 1, k2 = k - k1;\n";
         o << "   " << T << " y = (p * __builtin_bit_cast(" << T << ", (k1 + " << t.bias << ") << " << t.shift << ")) * __builtin_bit_cast(" << T
           << ", (k2 + " << t.bias << ") << " << t.shift << ");\n";
         o << "   y = a > " << c << "(" << t.xmax << ") ? " << c << "(__builtin_huge_val" << t.sfx << "()) : y;\n";
         o << "   return a != a ? a : y;\n}\n";
      }
      if (has[FZ_IR_LOG]) {
         // the fdlibm scheme: a = m 2^e, m in [sqrt(1/2), sqrt 2), through the exponent bits (subnormals scaled first, exactly)
         const bool dbl = &t == &tys[1];
         const char* L = dbl ? "LL" : "";
         const char *minn = dbl ? "0x0010000000000000" : "0x00800000", *scale = dbl ? "0x1p54" : "0x1p25f", *sbits = dbl ? "54" : "25",
                    *off = dbl ? "0x00095f619980c433" : "0x004afb0d", *mant = dbl ? "0x000fffffffffffff" : "0x007fffff",
                    *rh = dbl ? "0x3fe6a09e667f3bcd" : "0x3f3504f3";
         const std::vector<const char*> lg = dbl ? std::vector<const char*>{"0x1.5555555555558p-1", "0x1.9999999995204p-2", "0x1.2492492e09d1ap-2", "0x1.c71c62c63e016p-3",
                                                                         "0x1.7462bd8e53c17p-3", "0x1.39fd39474ad34p-3", "0x1.2b6686d1072f3p-3"} : std::vector<const char*>{"0x1.555556p-1f", "0x1.9999ecp-2f", "0x1.245c0ap-2f", "0x1.dddadep-3f"};
         auto ic = [&](const char* v) { return "(" + I + ")(" + v + L + ")"; };
         head("fz_log", false);
         o << "   // f = m - 1, s = f / (2 + f), log m = f - (h - s (h + R(s^2))), h = f^2 / 2; + e ln2 in two parts (e ln2_hi exact)\n";
         o << "   const auto sub = __builtin_bit_cast(" << I << ", a) < " << ic(minn) << ";   // subnormal (or zero, negative: overridden below)\n";
         o << "   const " << T << " x = sub ? a * " << c << "(" << scale << ") : a;\n";
         o << "   const " << I << " ix = __builtin_bit_cast(" << I << ", x) + " << ic(off) << ";\n";
         o << "   const " << I << " e = ((ix >> " << t.shift << ") - " << ic(t.bias) << ") - (sub ? " << ic(sbits) << " : " << ic("0") << ");\n";
         o << "   const " << T << " m = __builtin_bit_cast(" << T << ", (ix & " << ic(mant) << ") + " << ic(rh) << ");\n";
         o << "   const " << T << " f = m - " << c << "(1);\n";
         o << "   const " << T << " s = f / (" << c << "(2) + f);\n";
         o << "   const " << T << " z = s * s;\n";
         o << "   const " << T << " w = z * z;\n";
         // R = z (L1 + w (L3 + ..)) + w (L2 + w (L4 + ..)): lg[] holds L1, L2, ..
         for (int par = 0; par < 2; ++par) {
            std::vector<const char*> cs;
            for (size_t k = (size_t)par; k < lg.size(); k += 2) cs.push_back(lg[k]);
            const char* nm = par ? "t1" : "t2";
            o << "   " << T << " " << nm << " = " << c << "(" << cs.back() << ");\n";
            for (size_t k = cs.size() - 1; k-- > 0;) o << "   " << nm << " = " << c << "(" << cs[k] << ") + w * " << nm << ";\n";
         }
         o << "   const " << T << " R = z * t2 + w * t1;\n";
         o << "   const " << T << " h = (" << c << "(0.5) * f) * f;\n";
         o << "   const " << T << " ef = FZ_CVT(e, " << T << ");\n";
         o << "   const " << T << " u = s * (h + R) + ef * " << c << "(" << t.ln2lo << ");\n";
         o << "   " << T << " y = ef * " << c << "(" << t.ln2hi << ") + (f - (h - u));\n";
         o << "   y = a == " << c << "(__builtin_huge_val" << t.sfx << "()) ? a : y;\n";
         o << "   y = a < " << c << "(0) ? " << c << "(__builtin_nan" << t.sfx << "(\"\")) : y;\n";
         o << "   y = a == " << c << "(0) ? " << c << "(-__builtin_huge_val" << t.sfx << "()) : y;\n";
         o << "   return a != a ? a : y;\n}\n";
      }
      if (has[FZ_IR_TANH]) {
         head("fz_tanh", false);
         o << "   // odd: f(|a|) with the sign bit of a put back; |a| < 0.55: |a| + |a| (z P(z)), z = a^2; else 1 - 2 / (exp(2|a|) + 1); saturated: 1\n";
         o << "   const " << T << " x = __builtin_bit_cast(" << T << ", __builtin_bit_cast(" << I << ", a) & ~" << t.sign << ");\n";
         o << "   const " << T << " z = x * x;\n";
         o << "   " << T << " p = " << c << "(" << t.p[0] << ");\n";
         for (size_t k = 1; k < t.p.size(); ++k) o << "   p = " << c << "(" << t.p[k] << ") + z * p;\n";
         o << "   const " << T << " ys = x + x * (z * p);\n";
         o << "   const " << T << " xc = x > " << c << "(" << t.sat << ") ? " << c << "(" << t.sat << ") : x;\n";
         o << "   const " << T << " yb = " << c << "(1) - " << c << "(2) / (fz_exp(xc + xc) + " << c << "(1));\n";
         o << "   " << T << " y = x < " << c << "(" << t.sw << ") ? ys : yb;\n";
         o << "   y = x > " << c << "(" << t.sat << ") ? " << c << "(1) : y;\n";
         o << "   y = __builtin_bit_cast(" << T << ", __builtin_bit_cast(" << I << ", y) | (__builtin_bit_cast(" << I << ", a) & " << t.sign << "));\n";
         o << "   return a != a ? a : y;\n}\n";
      }
   }
}

// the frame kernels' body: struct fz_graph with the graph's state and step(), one sample of the whole graph
static std::string gen_body_frames(const Graph& g, const Variant& v)
{
   std::ostringstream o;
   auto val = [&](uint32_t id) { return "v" + std::to_string(id); };
   auto reg = [&](size_t line, uint32_t age) { return "r" + std::to_string(line) + "_" + std::to_string(age); };
   // slot of ring position `pos` (an unsigned expression that may have wrapped below zero by at most a ring's size: callers write
   // `n - delay`, `0u - 1u - j`): a mask for power-of-two rings, else a modulo of the position shifted up by a multiple of the size
   // that the wrap cannot reach (2^32 is not a multiple of the size, so the wrapped value itself must not be reduced)
   auto ring_idx = [&](const Line& l, const std::string& pos) {
      if ((l.lds_size & (l.lds_size - 1)) == 0) return "((" + pos + ") & " + std::to_string(l.lds_size - 1) + "u)";
      return "fz_ring_mod<" + std::to_string(l.lds_size) + "u>(" + pos + ")";
   };
   const RingPlan rp = ring_plan(g, v);
   // (vectorised rings: float offset of line l's row of this lane = (floats of the lines before it) * FZ_BLOCK + tid * (floats per row))
   std::vector<uint32_t> ring_before(g.lines.size(), 0), ring_row(g.lines.size(), 0);
   if (rp.vec) {
      uint32_t acc = 0;
      for (size_t l = 0; l < g.lines.size(); ++l)
         if (g.lines[l].in_lds) {
            ring_before[l] = acc;
            ring_row[l] = (g.lines[l].lds_size + rp.pad) * v.P;
            acc += ring_row[l];
         }
   }
   auto line_index = [&](const Line& l) { return (size_t)(&l - g.lines.data()); };
   auto ring_base = [&](const Line& l) {
      const size_t li = line_index(l);
      return "(" + std::to_string(ring_before[li]) + "u * FZ_BLOCK + tid * " + std::to_string(ring_row[li]) + "u)";
   };
   auto ring_at = [&](const Line& l, const std::string& pos) {
      if (rp.vec) return "(*reinterpret_cast<V*>(reinterpret_cast<float*>(ring) + " + ring_base(l) + " + " + ring_idx(l, pos) + " * " + std::to_string(v.P) + "u))";
      return "ring[(" + std::to_string(l.lds_slot0) + "u + " + ring_idx(l, pos) + ") * FZ_BLOCK + tid]";
   };
   auto ring_vec_at = [&](const Line& l, const std::string& pos) {      // 16 bytes = 4 / P consecutive slots of the lane, `pos` on that grid
      return "(*reinterpret_cast<fz_f4*>(reinterpret_cast<float*>(ring) + " + ring_base(l) + " + " + ring_idx(l, pos) + " * " + std::to_string(v.P) + "u))";
   };

   // a double ring keeps low and high words in two float rings of lds_size slots each
   auto ring_hi = [&](const Line& l, const std::string& pos) {
      return "ring[(" + std::to_string(l.lds_slot0 + l.lds_size) + "u + " + ring_idx(l, pos) + ") * FZ_BLOCK + tid]";
   };
   o << "// generated by libflowz_hip -- graph body: " << g.nodes.size() << " nodes, " << g.n_ops
     << " float32 ops/sample, " << g.lines.size() << " delay lines, " << g.n_state << " state floats\n";
   // (coefficient VALUES are not part of the text: they travel in the kernarg, and graphs that differ only in
   // literal values share one code object and one kernel-cache entry)
   o << "__device__ __forceinline__ V fz_div(V a, V b) { return a / b; }\n";
   o << "__device__ __forceinline__ VD fz_div(VD a, VD b) { return a / b; }\n";
   bool has_cmp = false;
   for (const Node& nd : g.nodes) has_cmp = has_cmp || is_cmp(nd.kind);
   if (has_cmp) {
      // the comparison operators of C++ on the streams of a lane: 1.0f / 0.0f (IEEE: every comparison with a NaN is false, != true); operands in
      // their common type.  Part of the GRAPH's text: kernels of graphs without comparisons keep their code.
      o << "template <int K, typename T> __device__ __forceinline__ bool fz_cmp1(T a, T b) { return ";
      for (const OpSpelling& s : kOps)
         if (is_cmp(s.kind)) o << (s.kind < FZ_IR_NE ? "K == " + std::to_string(s.kind) + " ? " : std::string()) << "a " << s.op << " b" << (s.kind < FZ_IR_NE ? " : " : "; }\n");
      o << "#if FZ_P == 1\n";
      o << "template <int K> __device__ __forceinline__ V fz_cmp(V a, V b) { return fz_cmp1<K>(a, b) ? 1.f : 0.f; }\n";
      o << "template <int K> __device__ __forceinline__ V fz_cmp(VD a, VD b) { return fz_cmp1<K>(a, b) ? 1.f : 0.f; }\n";
      o << "#else\n";
      for (const char* T : {"V", "VD"})
         o << "template <int K> __device__ __forceinline__ V fz_cmp(" << T << " a, " << T << " b)\n{\n   V r;\n#pragma unroll\n   for (int j = 0; j < FZ_P; ++j) r[j] = fz_cmp1<K>(a[j], b[j]) ? 1.f : 0.f;\n   return r;\n}\n";
      o << "#endif\n";
   }
   emit_functions(o, g);
   // operand `id` as seen by a node of type f64/f32 (C++ usual arithmetic conversions: float -> double is exact)
   auto opnd = [&](uint32_t id, bool want64) {
      return (want64 && !g.nodes[id].f64) ? "fz_cvt_d(" + val(id) + ")" : val(id);
   };
   // value of node `id` as float32 (delay lines and output frames are float: flowz.hpp:1245, rotate_push_back :130-137)
   auto as_f32 = [&](uint32_t id) { return g.nodes[id].f64 ? "fz_cvt_f(" + val(id) + ")" : val(id); };
   o << "struct fz_graph {\n";
   for (size_t l = 0; l < g.lines.size(); ++l) {
      const Line& L = g.lines[l];
      if (L.in_lds) {
         o << "   // line " << l << ": node " << L.src << ", depth " << L.depth << " -> LDS ring slots ["
           << L.lds_slot0 << ", " << L.lds_slot0 + L.lds_size << ")\n";
         continue;
      }
      if (L.far) {
         o << "   // line " << l << ": node " << L.src << ", depth " << L.depth << " -> ring in HBM: state rows ["
           << L.row0 << ", " << L.row0 + L.depth << "), phase in row " << L.phase_row << "\n";
         continue;
      }
      o << (L.f64 ? "   VD" : "   V");
      for (uint32_t a = 1; a <= L.depth; ++a) o << (a > 1 ? ", " : " ") << reg(l, a);
      o << ";   // line " << l << ": node " << L.src << " delayed by 1.." << L.depth << (L.f64 ? " (double state)" : "") << "\n";
   }
   for (uint32_t k = 0; k < g.n_param; ++k) o << "   V p" << k << ";\n";
   const std::vector<RingRead> reads = ring_reads(g, v, rp);
   auto read_of = [&](uint32_t line, uint32_t d) {            // index of that read in `reads`, reads.size(): read in place
      size_t k = 0;
      while (k < reads.size() && !(reads[k].line == line && reads[k].d == d)) ++k;
      return k;
   };
   if (rp.vec) {
      for (size_t k = 0; k < reads.size(); ++k)
         o << "   fz_f4 lr" << k << "[" << reads[k].nv << "];   // line " << reads[k].line << " read " << reads[k].d
           << " samples back: the sub-chunk's slots as 16-byte vectors, the first value " << reads[k].m << " slots in\n";
      for (size_t l = 0; l < g.lines.size(); ++l)
         if (g.lines[l].in_lds) o << "   fz_f4 wb" << l << "[" << rp.G / rp.TW << "];   // the sub-chunk's pushes of line " << l << "\n";
   } else {
      for (size_t k = 0; k < reads.size(); ++k)
         o << "   V lr" << k << "[FZ_U];   // line " << reads[k].line << " read " << reads[k].d << " samples back, the steps of the chunk at hand\n";
   }
   o << "   const float* mod = nullptr;   // sample-rate modulators [n_mod][mod_stride], set by the kernel (row 0 of the block)\n";
   o << "   unsigned mod_stride = 0;\n";
   // far lines: ring geometry for the skeleton, shadow registers for their short reads
   auto fidx = [&](size_t line) {
      for (size_t k = 0; k < g.far_lines.size(); ++k)
         if (g.far_lines[k] == line) return k;
      fail(FZ_E_GRAPH, "internal: not a far line");
   };
   auto shadow = [&](size_t line, uint32_t age) { return "fs" + std::to_string(line) + "_" + std::to_string(age); };
   if (!g.far_lines.empty()) {
      auto table = [&](const char* name, size_t n, auto get) {
         o << "   static constexpr unsigned " << name << "[" << std::max<size_t>(n, 1) << "] = {";
         for (size_t k = 0; k < std::max<size_t>(n, 1); ++k) o << (k ? ", " : "") << (k < n ? get(k) : 0u);
         o << "};\n";
      };
      table("fw_row0", g.far_lines.size(), [&](size_t k) { return g.lines[g.far_lines[k]].row0; });
      table("fw_depth", g.far_lines.size(), [&](size_t k) { return g.lines[g.far_lines[k]].depth; });
      table("fw_phase_row", g.far_lines.size(), [&](size_t k) { return g.lines[g.far_lines[k]].phase_row; });
      table("fr_line", g.far_reads.size(), [&](size_t k) { return (uint32_t)fidx(g.far_reads[k].line); });
      table("fr_n", g.far_reads.size(), [&](size_t k) { return g.far_reads[k].n; });
      for (uint32_t li : g.far_lines)
         if (g.lines[li].shadow) {
            o << "   V";
            for (uint32_t a = 1; a <= g.lines[li].shadow; ++a) o << (a > 1 ? ", " : " ") << shadow(li, a);
            o << ";   // newest values of far line " << li << " (node " << g.lines[li].src << ")\n";
         }
   }

   // ---- per-stream coefficients
   o << "   __device__ __forceinline__ void load_params(const float* pp, size_t ns, unsigned soff)\n   {\n";
   o << "      (void)pp; (void)ns; (void)soff;\n";
   for (uint32_t k = 0; k < g.n_param; ++k)
      o << "      p" << k << " = fz_ld_row(pp + (size_t)" << k << " * ns, soff, ns);\n";
   o << "   }\n";

   // ---- the state rows of line l, in (load_state) or out (store_state): row (row0 + j) holds the wire's value at t-1-j, a double
   // line's low and high words in rows (row0 + 2j, row0 + 2j + 1).  A register line is written out row by row; an LDS ring is a loop
   // over j, its value of age j + 1 at ring position `n - 1u - j` (n: the samples done, "0u" for the state in)
   auto state_rows = [&](size_t l, bool in, const std::string& n) {
      const Line& L = g.lines[l];
      const std::string fn = std::string(in ? "fz_ld_row" : "fz_st_row") + (L.f64 ? "64" : ""), args = L.f64 ? ", soff" : ", soff, ns";
      auto move = [&](const char* ind, const std::string& row, const std::string& value) {
         if (in) o << ind << value << " = " << fn << "(st + (size_t)" << row << " * ns" << args << ");\n";
         else o << ind << fn << "(st + (size_t)" << row << " * ns" << args << ", " << value << ");\n";
      };
      if (!L.in_lds) {
         for (uint32_t j = 0; j < L.depth; ++j) move("      ", std::to_string(L.row0 + (L.f64 ? 2 : 1) * j), reg(l, j + 1));
         return;
      }
      const std::string row = "(" + std::to_string(L.row0) + (L.f64 ? "u + 2u * j)" : "u + j)"), pos = n + " - 1u - j";
      o << "      for (unsigned j = 0; j < " << L.depth << "u; ++j)" << (L.f64 && in ? " {\n" : "\n");
      if (!L.f64) move("         ", row, ring_at(L, pos));
      else if (!in) move("         ", row, "fz_join_d(" + ring_at(L, pos) + ", " + ring_hi(L, pos) + ")");
      else {
         move("         ", row, "const VD d_");
         o << "         " << ring_at(L, pos) << " = fz_lo_d(d_);\n";
         o << "         " << ring_hi(L, pos) << " = fz_hi_d(d_);\n";
         o << "      }\n";
      }
   };
   o << "   __device__ __forceinline__ void load_state(const float* st, size_t ns, unsigned soff, V* ring, unsigned tid, const unsigned* ph)\n   {\n";
   o << "      (void)st; (void)ns; (void)soff; (void)ring; (void)tid; (void)ph;\n";
   for (size_t l = 0; l < g.lines.size(); ++l) {
      const Line& L = g.lines[l];
      if (!L.far) state_rows(l, true, "0u");
      else   // the newest values sit just behind the ring phase: age j+1 at slot (ph - 1 - j) mod D
         for (uint32_t j = 0; j < L.shadow; ++j)
            o << "      " << shadow(l, j + 1) << " = fz_ld_row(st + (size_t)(" << L.row0 << "u + (ph[" << fidx(l) << "] + " << (L.depth - 1 - j)
              << "u) % " << L.depth << "u) * ns, soff, ns);\n";
   }
   o << "   }\n";

   // ---- state out after n_done samples
   o << "   __device__ __forceinline__ void store_state(float* st, size_t ns, unsigned soff, V* ring, unsigned tid, unsigned n_done)\n   {\n";
   o << "      (void)st; (void)ns; (void)soff; (void)ring; (void)tid; (void)n_done;\n";
   for (size_t l = 0; l < g.lines.size(); ++l)
      if (!g.lines[l].far) state_rows(l, false, "n_done");   // (a far line's ring rows are written sample by sample)
   o << "   }\n";

   // ---- one sample
   o << "   // hr: values of the far delayed reads of this sample (prefetched from the HBM rings); hw: values to append to the rings\n";
   o << "   // mv / mvs: this sample's modulator values, modulator k at mv[k * mvs]\n";
   o << "   // the LDS ring reads of the chunk that starts at sample n0 (see lr<k> above)\n";
   o << "   __device__ __forceinline__ void ring_prefetch(V* ring, unsigned tid, unsigned n0)\n   {\n";
   o << "      (void)ring; (void)tid; (void)n0;\n";
   if (rp.vec) {
      // n0: first sample of the sub-chunk (a multiple of FZ_RING_G); vector j of read k starts at sample n0 - d - m + j * (4 / P)
      for (size_t k = 0; k < reads.size(); ++k)
         for (uint32_t j = 0; j < reads[k].nv; ++j)
            o << "      lr" << k << "[" << j << "] = " << ring_vec_at(g.lines[reads[k].line], "n0 + " + std::to_string(j * rp.TW) + "u - " + std::to_string(reads[k].d + reads[k].m) + "u") << ";\n";
   } else if (!reads.empty()) {
      o << "      _Pragma(\"unroll\") for (int u = 0; u < FZ_U; ++u)\n      {\n";
      for (size_t k = 0; k < reads.size(); ++k)
         o << "         lr" << k << "[u] = " << ring_at(g.lines[reads[k].line], "n0 + (unsigned)u - " + std::to_string(reads[k].d) + "u") << ";\n";
      o << "      }\n";
   }
   o << "   }\n";
   o << "   // the pushes of the sub-chunk that started at sample n0, kept in registers by its steps: 16 bytes per store\n";
   o << "   __device__ __forceinline__ void ring_flush(V* ring, unsigned tid, unsigned n0)\n   {\n";
   o << "      (void)ring; (void)tid; (void)n0;\n";
   if (rp.vec)
      for (size_t l = 0; l < g.lines.size(); ++l)
         if (g.lines[l].in_lds)
            for (uint32_t j = 0; j < rp.G / rp.TW; ++j)
               o << "      " << ring_vec_at(g.lines[l], "n0 + " + std::to_string(j * rp.TW) + "u") << " = wb" << l << "[" << j << "];\n";
   o << "   }\n";
   o << "   // u: the step's position in the chunk whose ring reads were prefetched (ring_prefetch), or -1: read the rings in place\n";
   o << "   __device__ __forceinline__ void step(const V* x, VO* y, const float* c, const double* cd, V* ring, unsigned tid, unsigned n, const V* hr, V* hw, const float* mv, unsigned mvs, int u = -1)\n   {\n";
   o << "      (void)x; (void)c; (void)cd; (void)ring; (void)tid; (void)n; (void)hr; (void)hw; (void)mv; (void)mvs; (void)u;\n";
   for (size_t id = 0; id < g.nodes.size(); ++id) {
      const Node& nd = g.nodes[id];
      const bool d = nd.f64;
      o << "      const " << (d ? "VD " : "V ") << val((uint32_t)id) << " = ";
      switch (nd.kind) {
         case FZ_IR_INPUT:
            if (d) o << "fz_join_d(x[" << nd.a << "], x[" << nd.a + 1 << "])";     // a double input wire: (low word, high word) slots
            else o << "x[" << nd.a << "]";
            break;
         case FZ_IR_CONST:
            if (d) o << "(VD)(cd[" << nd.a << "])";
            else o << "(V)(c[" << nd.a << "])";
            break;
         case FZ_IR_PARAM: o << "p" << nd.a; break;
         case FZ_IR_MOD: o << "(V)(fz_uniform_f(mv[" << nd.a << "u * mvs]))"; break;     // this sample's value of modulator a: wave-uniform (a scalar load, or a value the kernel prefetched with the chunk's rows)
         case FZ_IR_DELAY: {
            const int l = g.line_of_node[nd.a];
            const Line& L = g.lines[(size_t)l];
            if (L.far) {
               if (nd.b <= L.shadow) o << shadow((size_t)l, nd.b);
               else {
                  size_t r = 0;
                  while (r < g.far_reads.size() && !(g.far_reads[r].line == (uint32_t)l && g.far_reads[r].n == nd.b)) ++r;
                  o << "hr[" << r << "]";
               }
            } else if (!L.in_lds) o << reg((size_t)l, nd.b);
            else if (L.f64) o << "fz_join_d(" << ring_at(L, "n - " + std::to_string(nd.b) + "u") << ", " << ring_hi(L, "n - " + std::to_string(nd.b) + "u") << ")";
            else {
               const size_t k = read_of((uint32_t)l, nd.b);
               if (k < reads.size() && rp.vec)
                  o << "(u >= 0 ? fz_ring_pick(lr" << k << ", " << reads[k].m << " + (u % " << rp.G << ")) : " << ring_at(L, "n - " + std::to_string(nd.b) + "u") << ")";
               else if (k < reads.size()) o << "(u >= 0 ? lr" << k << "[u] : " << ring_at(L, "n - " + std::to_string(nd.b) + "u") << ")";
               else o << ring_at(L, "n - " + std::to_string(nd.b) + "u");
            }
            break;
         }
         default: {
            // compared in double when one operand is (the node itself is a float); every other operation in the node's own type
            const bool wide = is_cmp(nd.kind) ? g.nodes[nd.a].f64 || g.nodes[nd.b].f64 : d;
            const std::string e = op_expr(nd.kind, true, [&](uint32_t k, bool common) { return common ? opnd(operand(nd, k), wide) : val(operand(nd, k)); });
            if (e.empty()) fail(FZ_E_GRAPH, "internal: unknown IR node kind");
            o << e;
         }
      }
      o << ";\n";
   }
   for (size_t j = 0; j < g.outputs.size(); ++j) {
      const uint32_t id = g.outputs[j];
      if (g.out_part[j] >= 3 && (g.out_part[j] & 1)) o << "      y[" << j << "] = fz_lo_d(" << val(id) << ");\n";   // typed: a double (part), low word
      else if (g.out_part[j] >= 4) o << "      y[" << j << "] = fz_hi_d(" << val(id) << ");\n";
      else if (v.flags & FZ_VF_OUT_F64) o << "      y[" << j << "] = " << (g.nodes[id].f64 ? val(id) : "fz_cvt_d(" + val(id) + ")") << ";\n";
      else o << "      y[" << j << "] = " << as_f32(id) << ";\n";
   }
   // pushes last: every read above saw the values of previous samples (flowz.hpp:994, :1067)
   for (size_t l = 0; l < g.lines.size(); ++l) {
      const Line& L = g.lines[l];
      if (L.far) {
         o << "      hw[" << fidx(l) << "] = " << as_f32(L.src) << ";\n";
         shift_line(o, L.shadow, [&](uint32_t a) { return shadow(l, a); }, as_f32(L.src));
      } else if (!L.in_lds) {
         shift_line(o, L.depth, [&](uint32_t a) { return reg(l, a); }, L.f64 ? val(L.src) : as_f32(L.src));
      } else if (L.f64) {
         o << "      " << ring_at(L, "n") << " = fz_lo_d(" << val(L.src) << ");\n";
         o << "      " << ring_hi(L, "n") << " = fz_hi_d(" << val(L.src) << ");\n";
      } else if (rp.vec) {
         o << "      if (u >= 0) fz_ring_put(wb" << l << ", u % " << rp.G << ", " << as_f32(L.src) << ");\n";
         o << "      else " << ring_at(L, "n") << " = " << as_f32(L.src) << ";\n";
      } else {
         o << "      " << ring_at(L, "n") << " = " << as_f32(L.src) << ";\n";
      }
   }
   o << "   }\n";
   o << "};\n";
   return o.str();
}

// the wave split: the parts of the graph, each a stage-packed body of its own (struct fz_r0::fz_graph, fz_r1::fz_graph, ...)
static std::string gen_body_waves(const Graph& g, uint32_t W)
{
   const std::vector<Graph>* roles = g.wave_roles(W);
   if (!roles) fail(FZ_E_UNSUPPORTED, "wave split: the graph is not that many isomorphic parts in series");
   std::string s;
   for (uint32_t r = 0; r < 4; ++r) {
      if (r < W) s += "namespace fz_r" + std::to_string(r) + " {\n" + gen_body_skew((*roles)[r], (*roles)[r].split) + "}\n#undef FZ_NSEG\n";
      else s += "namespace fz_r" + std::to_string(r) + " { typedef fz_r0::fz_graph fz_graph; }\n";   // (unused: keeps the dispatch uniform)
   }
   return s;
}

std::string gen_body(const Graph& g, const Variant& v)
{
   if (v.flags & FZ_VF_ADJOINT)
      // (the far states kernel calls fwd() alone, which is one text on either path of bwd(): it takes the per-row one)
      return gen_adjoint_body(g, (v.flags & FZ_VF_ADJOINT_LOSS) != 0, (v.flags & FZ_VF_ADJOINT_RING) != 0,
                              !(v.flags & FZ_VF_ADJOINT_FAR) ? 0 : !(v.flags & FZ_VF_STATES) && far_fast_path(g, v.U) ? 2 : 1);
   if (const uint32_t W = ws_parts(v.flags)) return gen_body_waves(g, W);
   if (v.flags & FZ_VF_STAGE_PACK) return gen_body_skew(g, g.split);
   return gen_body_frames(g, v);
}

// Stage-packed body (FZ_VF_STAGE_PACK, one stream per lane): K isomorphic segments, segment j at
// time t-j; stream i of packed float2 operations carries (segment i, segment i + K/2), so that the
// packed output of stream i-1 IS the packed input of stream i in the next step (no shuffles).
static std::string gen_body_skew(const Graph& g, const StageSplit& sp)
{
   if (!sp.ok) fail(FZ_E_UNSUPPORTED, "graph is not a series of isomorphic segments: stage packing does not apply");
   const uint32_t K = sp.K, NS = K / 2, M = sp.m, NA = K * M;   // segments, packed streams, atoms per segment, atoms in all
   std::ostringstream o;
   std::map<std::vector<uint32_t>, size_t> tid;
   for (size_t k = 0; k < sp.tuples.size(); ++k) tid[sp.tuples[k]] = k;
   auto operand_tuple = [&](const std::vector<uint32_t>& t, bool second) {
      std::vector<uint32_t> r(K);
      for (uint32_t j = 0; j < K; ++j) r[j] = second ? g.nodes[t[j]].b : g.nodes[t[j]].a;
      return r;
   };
   auto sub_of = [&](const std::vector<uint32_t>& t) -> uint32_t {
      auto it = tid.find(t);
      if (it == tid.end()) fail(FZ_E_GRAPH, "internal: unmatched operand in stage packing");
      return sp.sub.empty() ? 0u : sp.sub[it->second];
   };
   std::map<std::pair<std::vector<uint32_t>, uint32_t>, size_t> lid;   // (source tuple, frame) -> packed line
   for (size_t l = 0; l < sp.lines.size(); ++l) lid[{sp.lines[l].srcs, sp.lines[l].frame}] = l;
   auto q = [&](size_t l, uint32_t i, uint32_t age) {
      return "q" + std::to_string(l) + "_" + std::to_string(i) + "_" + std::to_string(age);
   };
   auto cy = [&](uint32_t a, uint32_t i) { return "cy" + std::to_string(a) + "_" + std::to_string(i); };   // carry INTO atom a
   // the packed value of tuple t as atom `rs` of stream i sees it in this step: its own atom's fresh value, the carry that
   // brought the internal cut wire over from the atom before (one step ago), or a delayed read in the atom's own time frame
   auto w = [&](const std::vector<uint32_t>& t, uint32_t i, uint32_t rs = ~0u) -> std::string {
      auto it = tid.find(t);
      if (it == tid.end()) fail(FZ_E_GRAPH, "internal: unmatched operand in stage packing");
      const Node& n0 = g.nodes[t[0]];
      if (rs != ~0u && n0.kind == FZ_IR_DELAY) {
         auto li = lid.find({operand_tuple(t, false), rs});
         if (li == lid.end()) fail(FZ_E_GRAPH, "internal: delayed read without a line in the reader's time frame");
         return q(li->second, i, n0.b);
      }
      const bool leaf = n0.kind == FZ_IR_CONST || n0.kind == FZ_IR_PARAM || t[0] == sp.cuts[0];
      if (rs != ~0u && !leaf && sub_of(t) != rs) {
         if (rs == 0 || rs - 1 >= sp.icuts.size() || sp.icuts[rs - 1] != t)
            fail(FZ_E_GRAPH, "internal: an atom reads an earlier atom past its cut wire");
         return cy(rs, i);
      }
      return "w" + std::to_string(it->second) + "_" + std::to_string(i);
   };
   auto row_of = [&](uint32_t s, uint32_t j) -> long {
      const int l = g.line_of_node[s];
      if (l < 0 || j >= g.lines[(size_t)l].depth) return -1;
      return (long)g.lines[(size_t)l].row0 + j;
   };
   std::vector<uint32_t> root(K);
   for (uint32_t j = 0; j < K; ++j) root[j] = sp.cuts[j + 1];

   o << "// generated by libflowz_hip -- STAGE-PACKED graph body: " << K << " isomorphic segments of " << g.n_ops / K
     << " float32 ops, cut at nodes";
   for (uint32_t j = 1; j < K; ++j) o << " " << sp.cuts[j];
   o << "; segment j runs at time t-j, segments (i, i+" << NS << ") share packed stream i";
   if (M > 1) o << "; every segment is " << M << " atoms in series (atom a of segment j at time t-(j*" << M << "+a))";
   o << "\n#define FZ_NSEG " << NA << "   // skewed units in series (mask bits)\n";
   o << "struct fz_graph {\n";
   for (size_t l = 0; l < sp.lines.size(); ++l)
      for (uint32_t i = 0; i < NS; ++i) {
         o << "   fz_f2";
         for (uint32_t a = 1; a <= sp.lines[l].depth; ++a) o << (a > 1 ? ", " : " ") << q(l, i, a);
         o << ";   // (node " << sp.lines[l].srcs[i] << ", node " << sp.lines[l].srcs[i + NS] << ") delayed by 1.."
           << sp.lines[l].depth << "\n";
      }
   std::vector<size_t> ptuples;
   for (size_t k = 0; k < sp.tuples.size(); ++k)
      if (g.nodes[sp.tuples[k][0]].kind == FZ_IR_PARAM) ptuples.push_back(k);
   for (size_t k : ptuples)
      for (uint32_t i = 0; i < NS; ++i) o << "   fz_f2 pp" << k << "_" << i << ";\n";
   // scalar prefix (runs with segment 0): private delay lines and per-stream coefficients
   auto ps = [&](uint32_t l, uint32_t age) { return "ps" + std::to_string(l) + "_" + std::to_string(age); };
   std::vector<char> in_prefix(g.nodes.size(), 0);
   for (uint32_t v : sp.prefix) in_prefix[v] = 1;
   std::vector<char> is_prefix_line(g.lines.size(), 0);
   for (uint32_t l : sp.prefix_lines) {
      is_prefix_line[l] = 1;
      o << "   float";
      for (uint32_t a = 1; a <= g.lines[l].depth; ++a) o << (a > 1 ? ", " : " ") << ps(l, a);
      o << ";   // prefix line: node " << g.lines[l].src << "\n";
   }
   // scalar suffix (runs with the last segment): its private delay lines
   auto ss = [&](uint32_t l, uint32_t age) { return "ss" + std::to_string(l) + "_" + std::to_string(age); };
   std::vector<char> is_suffix_line(g.lines.size(), 0);
   for (uint32_t l : sp.suffix_lines) {
      is_suffix_line[l] = 1;
      o << "   float";
      for (uint32_t a = 1; a <= g.lines[l].depth; ++a) o << (a > 1 ? ", " : " ") << ss(l, a);
      o << ";   // suffix line: node " << g.lines[l].src << "\n";
   }
   std::vector<uint32_t> prefix_params;                   // per-stream coefficients of the scalar parts
   for (uint32_t v : sp.prefix)
      if (g.nodes[v].kind == FZ_IR_PARAM) prefix_params.push_back(g.nodes[v].a);
   for (uint32_t v : sp.suffix) {
      auto add_param = [&](uint32_t o) {
         if (g.nodes[o].kind == FZ_IR_PARAM && std::find(prefix_params.begin(), prefix_params.end(), g.nodes[o].a) == prefix_params.end())
            prefix_params.push_back(g.nodes[o].a);
      };
      add_param(v);
      const Node& nd = g.nodes[v];
      if (nd.kind >= FZ_IR_ADD && nd.kind <= FZ_IR_NEG) {
         add_param(nd.a);
         if (nd.kind != FZ_IR_NEG) add_param(nd.b);
      }
   }
   for (uint32_t k : prefix_params) o << "   float pf" << k << ";\n";
   o << "   const float* mod = nullptr;\n   unsigned mod_stride = 0;\n";
   o << "   fz_f2";
   for (uint32_t i = 0; i < NS; ++i) o << (i ? ", " : " ") << "cq" << i;
   o << ";   // cq_i: packed output of stream i = packed input of stream i+1 in the next step\n";
   for (uint32_t a = 1; a < M; ++a) {
      o << "   fz_f2";
      for (uint32_t i = 0; i < NS; ++i) o << (i ? ", " : " ") << cy(a, i);
      o << ";   // the internal cut wire in front of atom " << a << ", one step old\n";
   }

   o << "   __device__ __forceinline__ void load_params(const float* pp, size_t ns, unsigned soff)\n   {\n";
   o << "      (void)pp; (void)ns; (void)soff;\n";
   for (uint32_t i = 0; i < NS; ++i) o << "      cq" << i << " = (fz_f2){0.f, 0.f};\n";
   for (uint32_t a = 1; a < M; ++a)
      for (uint32_t i = 0; i < NS; ++i) o << "      " << cy(a, i) << " = (fz_f2){0.f, 0.f};\n";
   for (uint32_t k : prefix_params) o << "      pf" << k << " = fz_ld_f(pp + (size_t)" << k << " * ns, soff, ns);\n";
   for (size_t k : ptuples)
      for (uint32_t i = 0; i < NS; ++i)
         o << "      pp" << k << "_" << i << " = (fz_f2){fz_ld_f(pp + (size_t)" << g.nodes[sp.tuples[k][i]].a << " * ns, soff, ns), fz_ld_f(pp + (size_t)"
           << g.nodes[sp.tuples[k][i + NS]].a << " * ns, soff, ns)};\n";
   o << "   }\n";

   o << "   __device__ __forceinline__ void load_state(const float* st, size_t ns, unsigned soff, V* ring, unsigned tid, const unsigned* ph)\n   {\n";
   o << "      (void)st; (void)ns; (void)soff; (void)ring; (void)tid; (void)ph;\n";
   auto ld = [&](long r) { return r < 0 ? std::string("0.f") : "fz_ld_f(st + (size_t)" + std::to_string(r) + " * ns, soff, ns)"; };
   for (size_t l = 0; l < sp.lines.size(); ++l)
      for (uint32_t i = 0; i < NS; ++i)
         for (uint32_t j = 0; j < sp.lines[l].depth; ++j)
            o << "      " << q(l, i, j + 1) << " = (fz_f2){" << ld(row_of(sp.lines[l].srcs[i], j)) << ", "
              << ld(row_of(sp.lines[l].srcs[i + NS], j)) << "};\n";
   for (uint32_t l : sp.prefix_lines)
      for (uint32_t j = 0; j < g.lines[l].depth; ++j)
         o << "      " << ps(l, j + 1) << " = fz_ld_f(st + (size_t)" << (g.lines[l].row0 + j) << " * ns, soff, ns);\n";
   for (uint32_t l : sp.suffix_lines)
      for (uint32_t j = 0; j < g.lines[l].depth; ++j)
         o << "      " << ss(l, j + 1) << " = fz_ld_f(st + (size_t)" << (g.lines[l].row0 + j) << " * ns, soff, ns);\n";
   o << "   }\n";

   o << "   __device__ __forceinline__ void store_state(float* st, size_t ns, unsigned soff, V* ring, unsigned tid, unsigned n_done)\n   {\n";
   o << "      (void)st; (void)ns; (void)soff; (void)ring; (void)tid; (void)n_done;\n";
   for (size_t li = 0; li < g.lines.size(); ++li) {
      const Line& L = g.lines[li];
      for (uint32_t j = 0; j < L.depth; ++j) {
         if (is_prefix_line[li] || is_suffix_line[li]) {
            o << "      fz_st_f(st + (size_t)" << (L.row0 + j) << " * ns, soff, ns, " << (is_prefix_line[li] ? ps((uint32_t)li, j + 1) : ss((uint32_t)li, j + 1)) << ");\n";
            continue;
         }
         // every copy of a shared line holds the same values once all segments have caught up
         std::string src;
         for (size_t l = 0; l < sp.lines.size() && src.empty(); ++l)
            for (uint32_t p = 0; p < K && src.empty(); ++p)
               if (sp.lines[l].srcs[p] == L.src && j < sp.lines[l].depth) src = q(l, p % NS, j + 1) + (p >= NS ? ".y" : ".x");
         if (src.empty()) fail(FZ_E_GRAPH, "internal: delay line not covered by stage packing");
         o << "      fz_st_f(st + (size_t)" << (L.row0 + j) << " * ns, soff, ns, " << src << ");\n";
      }
   }
   o << "   }\n";

   o << "   // one step: segment j consumes/produces time t-j.  MASKED (prologue/epilogue steps only): bit j of\n";
   o << "   // `mask` says whether segment j runs; an idle segment keeps its delay lines and its carry.\n";
   o << "   template <bool MASKED>\n";
   o << "   __device__ __forceinline__ void step2(const V* x, VO* y, const float* c, unsigned mask)\n   {\n";
   o << "      (void)c; (void)mask;\n";
   // scalar prefix at the time of segment 0
   // a scalar part's delayed read of a wire the chain keeps packed lines of: the copy in the time frame of the atom the scalar
   // part runs with (prefix: atom 0 of segment 0; suffix: the last atom of the last segment)
   auto packed_comp_of = [&](uint32_t src, uint32_t age, uint32_t frame) -> std::string {
      for (size_t l = 0; l < sp.lines.size(); ++l)
         for (uint32_t pz = 0; pz < K; ++pz)
            if (sp.lines[l].frame == frame && sp.lines[l].srcs[pz] == src && age <= sp.lines[l].depth) return q(l, pz % NS, age) + (pz >= NS ? ".y" : ".x");
      fail(FZ_E_GRAPH, "internal: a scalar prefix / suffix reads a delay line that is not materialised in its time frame");
   };
   // an operation of the chain or of a scalar part: one of the kinds the split takes (fz_split.cpp: is_arith), x(k) its operand k
   auto arith = [&](const Node& nd, const std::function<std::string(uint32_t)>& x) {
      if (!is_arith(nd.kind)) fail(FZ_E_GRAPH, "internal: a node kind stage packing does not take");
      return op_expr(nd.kind, false, [&](uint32_t k, bool) { return x(k); });
   };
   for (uint32_t v : sp.prefix) {
      const Node& nd = g.nodes[v];
      const int l = nd.kind == FZ_IR_DELAY ? g.line_of_node[nd.a] : -1;
      o << "      const float u" << v << " = ";
      if (nd.kind == FZ_IR_INPUT) o << "x[0]";
      else if (nd.kind == FZ_IR_CONST) o << "c[" << nd.a << "]";
      else if (nd.kind == FZ_IR_PARAM) o << "pf" << nd.a;
      else if (nd.kind == FZ_IR_DELAY) o << (l >= 0 && is_prefix_line[(size_t)l] ? ps((uint32_t)l, nd.b) : packed_comp_of(nd.a, nd.b, 0));
      else o << arith(nd, [&](uint32_t k) { return "u" + std::to_string(operand(nd, k)); });
      o << ";\n";
   }
   const std::string chain_in = g.nodes[sp.cuts[0]].kind == FZ_IR_INPUT ? std::string("x[0]") : "u" + std::to_string(sp.cuts[0]);
   for (size_t k = 0; k < sp.tuples.size(); ++k) {
      const auto& t = sp.tuples[k];
      const Node& n0 = g.nodes[t[0]];
      if (n0.kind == FZ_IR_DELAY) continue;                                    // (read where it is used, in the reader's time frame)
      for (uint32_t i = 0; i < NS; ++i) {
         o << "      const fz_f2 w" << k << "_" << i << " = ";
         const Node& na = g.nodes[t[i]];
         const Node& nb = g.nodes[t[i + NS]];
         if (t[0] == sp.cuts[0]) {                                        // the chain's input wire
            if (i == 0) o << "(fz_f2){" << chain_in << ", cq" << NS - 1 << ".x};\n";   // segment 0 <- input / prefix, segment NS <- segment NS-1
            else o << "cq" << i - 1 << ";\n";                             // segments (i, i+NS) <- segments (i-1, i-1+NS)
            continue;
         }
         const uint32_t rs = sp.sub.empty() ? 0u : sp.sub[k];                 // the atom this operation belongs to
         if (n0.kind == FZ_IR_CONST) o << "(fz_f2){c[" << na.a << "], c[" << nb.a << "]}";
         else if (n0.kind == FZ_IR_PARAM) o << "pp" << k << "_" << i;
         else o << arith(n0, [&](uint32_t j) { return w(operand_tuple(t, j == 1), i, rs); });
         o << ";\n";
      }
   }
   if (sp.suffix.empty()) {
      o << "      y[0] = " << w(root, NS - 1) << ".y;\n";
   } else {
      // scalar suffix at the time of the last segment: what the output makes of the chain's end wire
      const uint32_t e = sp.cuts[K];
      auto sval = [&](uint32_t v) -> std::string {
         if (v == e) return w(root, NS - 1) + ".y";
         const Node& nd = g.nodes[v];
         if (nd.kind == FZ_IR_CONST) return "c[" + std::to_string(nd.a) + "]";
         if (nd.kind == FZ_IR_PARAM) return "pf" + std::to_string(nd.a);
         if (nd.kind == FZ_IR_DELAY && nd.a == e && std::find(sp.suffix.begin(), sp.suffix.end(), v) == sp.suffix.end())
            return packed_comp_of(e, nd.b, M - 1);                          // a delayed read of e shared with the chain
         return "z" + std::to_string(v);
      };
      for (uint32_t v : sp.suffix) {
         const Node& nd = g.nodes[v];
         if (nd.kind == FZ_IR_CONST || nd.kind == FZ_IR_PARAM) continue;
         const int l = nd.kind == FZ_IR_DELAY ? g.line_of_node[nd.a] : -1;
         o << "      const float z" << v << " = ";
         if (nd.kind == FZ_IR_DELAY) o << (l >= 0 && is_suffix_line[(size_t)l] ? ss((uint32_t)l, nd.b) : packed_comp_of(nd.a, nd.b, M - 1));
         else o << arith(nd, [&](uint32_t k) { return sval(operand(nd, k)); });
         o << ";\n";
      }
      o << "      y[0] = " << sval(g.outputs[0]) << ";\n";
   }
   // atom `a` of segment `seg` is mask bit seg * M + a
   auto act = [&](uint32_t seg, uint32_t a) { return "(!MASKED || ((mask >> " + std::to_string(seg * M + a) + ") & 1u))"; };
   for (size_t l = 0; l < sp.lines.size(); ++l)
      for (uint32_t i = 0; i < NS; ++i) {
         const uint32_t fr = sp.lines[l].frame;                               // the line lives in the time frame of atom fr: pushed when that atom runs
         shift_line(o, sp.lines[l].depth, [&](uint32_t a) { return q(l, i, a); }, w(sp.lines[l].srcs, i, fr), act(i, fr), act(i + NS, fr));
      }
   for (uint32_t a = 1; a < M; ++a)                                           // the internal cut wires travel on to the next atom
      for (uint32_t i = 0; i < NS; ++i) {
         const std::string cur = w(sp.icuts[a - 1], i);
         o << "      " << cy(a, i) << " = (fz_f2){" << act(i, a - 1) << " ? " << cur << ".x : " << cy(a, i) << ".x, " << act(i + NS, a - 1) << " ? "
           << cur << ".y : " << cy(a, i) << ".y};\n";
      }
   for (uint32_t l : sp.prefix_lines) {
      const Line& L = g.lines[l];
      const std::string cur = g.nodes[L.src].kind == FZ_IR_INPUT ? std::string("x[0]") : "u" + std::to_string(L.src);
      shift_line(o, L.depth, [&](uint32_t a) { return ps(l, a); }, cur, act(0, 0));
   }
   for (uint32_t l : sp.suffix_lines) {
      const Line& L = g.lines[l];
      const std::string cur = L.src == sp.cuts[K] ? w(root, NS - 1) + ".y" : "z" + std::to_string(L.src);
      shift_line(o, L.depth, [&](uint32_t a) { return ss(l, a); }, cur, act(K - 1, M - 1));
   }
   for (uint32_t i = 0; i < NS; ++i)
      o << "      cq" << i << " = (fz_f2){" << act(i, M - 1) << " ? " << w(root, i) << ".x : cq" << i << ".x, " << act(i + NS, M - 1) << " ? "
        << w(root, i) << ".y : cq" << i << ".y};\n";
   o << "   }\n";
   o << "};\n";
   return o.str();
}

std::string full_source(const Graph& g, const Variant& v)
{
   // single translation unit view (for inspection and for hashing the kernel cache key)
   std::string s;
   s += "// ==== fz_graph_config.h ====\n" + gen_config(g, v);
   s += "// ==== fz_graph_body.h ====\n" + gen_body(g, v);
   s += "// ==== fz_block_kernel.hip.inc ====\n";
   s += skeleton_source(v);
   return s;
}


// ---- the adjoint kernel (fz_kernel_adjoint.hip.inc, fz_grad.cpp) ----------------------------------------------------------------------
std::string gen_adjoint_config(const Graph& g, const Variant& v)
{
   std::ostringstream o;
   o << ((v.flags & FZ_VF_STATES) ? "// generated by libflowz_hip -- block-start-states kernel configuration\n" : "// generated by libflowz_hip -- adjoint kernel configuration\n");
   o << "#define FZ_NIN " << g.n_in << "\n";
   o << "#define FZ_NOUT " << g.n_out << "\n";
   o << "#define FZ_NCONST " << g.consts.size() << "\n";
   o << "#define FZ_NPARAM " << g.n_param << "\n";
   o << "#define FZ_NSTATE " << g.n_state << "\n";
   if (v.flags & FZ_VF_ADJOINT_RING) {
      const RingLayout rl = ring_layout(g);
      o << "#define FZ_NREG " << rl.n_reg() << "   // state rows of the lines in registers (depth <= " << kRegMaxDepth << ")\n";
      o << "#define FZ_NRL " << rl.n_rl() << "   // ring lines: delay lines in LDS\n";
      o << "#define FZ_NRR " << rl.n_rr() << "   // ring reads: distinct (ring line, delay) pairs\n";
      o << "#define FZ_RING_SLOTS " << rl.slots << "   // LDS slots per lane: the sum of the ring lines' depths\n";
      auto table = [&](const char* name, size_t n, const std::function<uint32_t(size_t)>& at, const char* what) {
         o << "static __device__ constexpr unsigned " << name << "[" << std::max<size_t>(n, 1) << "] = {";
         for (size_t i = 0; i < std::max<size_t>(n, 1); ++i) o << (i ? ", " : "") << (i < n ? at(i) : 0u) << "u";
         o << "};   // " << what << "\n";
      };
      table("fz_reg_row", rl.n_reg(), [&](size_t i) { return rl.reg_row[i]; }, "per register row: the caller's state row");
      table("fz_rl_row0", rl.n_rl(), [&](size_t i) { return g.lines[rl.rl_line[i]].row0; }, "per ring line: its first state row");
      table("fz_rl_depth", rl.n_rl(), [&](size_t i) { return g.lines[rl.rl_line[i]].depth; }, "per ring line: its depth = its LDS slots");
      table("fz_rl_slot0", rl.n_rl(), [&](size_t i) { return rl.rl_slot0[i]; }, "per ring line: its first LDS slot");
      table("fz_rr_line", rl.n_rr(), [&](size_t i) { return rl.reads[i].first; }, "per ring read: its ring line");
      table("fz_rr_delay", rl.n_rr(), [&](size_t i) { return rl.reads[i].second; }, "per ring read: its delay in samples");
      o << "#define FZ_FAR " << ((v.flags & FZ_VF_ADJOINT_FAR) ? 1 : 0) << "   // 1: the delay lines deeper than " << kLdsMaxDepth << " samples keep their rings in HBM\n";
      if (v.flags & FZ_VF_ADJOINT_FAR) {
         o << "#define FZ_NFL " << rl.n_fl() << "   // far lines: delay lines deeper than " << kLdsMaxDepth << " samples, rings in HBM\n";
         o << "#define FZ_NFR " << rl.n_fr() << "   // far reads: distinct (far line, delay) pairs\n";
         o << "#define FZ_FAR_SLOTS " << rl.far_slots << "   // rows of the adjoint ring in the workspace: the sum of the far lines' depths\n";
         if (!(v.flags & FZ_VF_STATES)) o << "#define FZ_FAR_FAST " << (far_fast_path(g, v.U) ? 1 : 0) << "   // 1: no slot is touched twice within a chunk -- the pending adjoints travel with the chunk's rows\n";
         table("fz_fl_row0", rl.n_fl(), [&](size_t i) { return g.lines[rl.fl_line[i]].row0; }, "per far line: its first state row");
         table("fz_fl_depth", rl.n_fl(), [&](size_t i) { return g.lines[rl.fl_line[i]].depth; }, "per far line: its depth = its ring slots");
         table("fz_fl_slot0", rl.n_fl(), [&](size_t i) { return rl.fl_slot0[i]; }, "per far line: its first row of the adjoint ring");
         table("fz_fl_phase_row", rl.n_fl(), [&](size_t i) { return g.lines[rl.fl_line[i]].phase_row; }, "per far line: the state row of its ring phase");
         table("fz_fr_line", rl.n_fr(), [&](size_t i) { return rl.far_reads[i].first; }, "per far read: its far line");
         table("fz_fr_delay", rl.n_fr(), [&](size_t i) { return rl.far_reads[i].second; }, "per far read: its delay in samples");
         if (v.flags & FZ_VF_STATES) table("fz_fr_ahead", rl.n_fr(), [&](size_t i) { return far_read_with_next_group(rl.far_reads[i].second, v.U) ? 1u : 0u; }, "per far read: 1 = requested with the next group's x rows");
         else table("fz_fr_chunked", rl.n_fr(), [&](size_t i) { return far_read_with_chunk(rl.far_reads[i].second, v.U) ? 1u : 0u; }, "per far read: 1 = sweep 1 requests it with the chunk's x rows");
      }
   }
   if (v.flags & FZ_VF_STATES) {
      o << "#define FZ_RING " << ((v.flags & FZ_VF_ADJOINT_RING) ? 1 : 0) << "   // 1: the delay lines deeper than " << kRegMaxDepth << " samples keep value rings in LDS\n";
      o << "#define FZ_U " << v.U << "   // rows per unrolled group of the forward recursion\n";
   }
   else o << "#define FZ_C " << v.U << "   // checkpoint rows: the chunk sweep 2 re-runs and walks backwards\n";
   if (!(v.flags & FZ_VF_STATES)) o << "#define FZ_LOSS " << ((v.flags & FZ_VF_ADJOINT_LOSS) ? 1 : 0) << "   // 1: dL/dy is formed in the kernel, from a target (the squared-error loss)\n";
   if (v.flags & FZ_VF_ADJOINT_SM) o << "#define FZ_R " << v.P << "   // rows per LDS patch of the stream-major frames\n";
   o << "#define FZ_BLOCK " << v.block << "\n";
   o << "#define FZ_KERNEL " << kernel_symbol(g, v) << "\n";
   return o.str();
}

// the node kinds the adjoint kernel takes: inputs, coefficients, delayed reads and float arithmetic (INPUT .. NEG), the comparisons
// and the graph functions (LT .. LOG) -- not the conversions, modulators, |a| < |b| and selections between them
bool adjoint_takes(uint32_t kind) { return (kind >= FZ_IR_INPUT && kind <= FZ_IR_NEG) || (kind >= FZ_IR_LT && kind <= FZ_IR_LOG); }

// how the ring adjoint kernel lays a graph out (fz_internal.hpp: RingLayout)
int RingLayout::read_index(uint32_t ring_line, uint32_t delay) const
{
   for (size_t i = 0; i < reads.size(); ++i)
      if (reads[i].first == ring_line && reads[i].second == delay) return (int)i;
   return -1;
}

int RingLayout::far_read_index(uint32_t far_line, uint32_t delay) const
{
   for (size_t i = 0; i < far_reads.size(); ++i)
      if (far_reads[i].first == far_line && far_reads[i].second == delay) return (int)i;
   return -1;
}

RingLayout ring_layout(const Graph& g)
{
   RingLayout rl;
   for (size_t l = 0; l < g.lines.size(); ++l) {
      const Line& L = g.lines[l];
      rl.far_of_line.push_back(L.far ? (int)rl.fl_line.size() : -1);
      if (L.far) {                                          // (neither register rows nor LDS slots: FZ_FAR in fz_kernel_adjoint_ring.hip.inc)
         rl.reg0.push_back(-1);
         rl.ring_of_line.push_back(-1);
         rl.fl_line.push_back((uint32_t)l);
         rl.fl_slot0.push_back(rl.far_slots);
         rl.far_slots += L.depth;
      } else if (L.in_lds) {
         rl.reg0.push_back(-1);
         rl.ring_of_line.push_back((int)rl.rl_line.size());
         rl.rl_line.push_back((uint32_t)l);
         rl.rl_slot0.push_back(rl.slots);
         rl.slots += L.depth;
      } else {
         rl.reg0.push_back((int)rl.reg_row.size());
         rl.ring_of_line.push_back(-1);
         for (uint32_t a = 0; a < L.depth; ++a) rl.reg_row.push_back(L.row0 + a);
      }
   }
   for (const Node& nd : g.nodes) {
      if (nd.kind != FZ_IR_DELAY) continue;
      const int k = rl.ring_of_line[(size_t)g.line_of_node[nd.a]], f = rl.far_of_line[(size_t)g.line_of_node[nd.a]];
      if (k >= 0 && rl.read_index((uint32_t)k, nd.b) < 0) rl.reads.emplace_back((uint32_t)k, nd.b);
      if (f >= 0 && rl.far_read_index((uint32_t)f, nd.b) < 0) rl.far_reads.emplace_back((uint32_t)f, nd.b);
   }
   return rl;
}

// ---- the far kernel's two static rules (their one home; fz_internal.hpp declares them, include/flowz_hip.h states them) ----------------
// Sweep 1 reads a far line's values back from the tape rows it wrote itself.  A read at least C rows old reads a row written before
// its chunk began, whichever row of the chunk asks: it is requested with the chunk's x rows.  A younger read is a load of its own in
// front of its row (the forward shortens the chunk instead, below kFarMinDelay: here the chunk is the checkpoint stride and stays).
bool far_read_with_chunk(uint32_t delay, uint32_t C) { return delay >= C; }

// The far states kernel (fz_kernel_states.hip.inc with FZ_FAR) requests the x rows of the NEXT group of U rows before the current group runs.
// A far read may travel with them when the slot it reads was written before that request is issued, whichever row of the next group
// asks: the youngest source row is that of the group's last row, t0 + 2U - 1 - delay, and it must lie before t0.  A younger read is a
// load of its own in front of its row.
bool far_read_with_next_group(uint32_t delay, uint32_t U) { return delay >= 2 * U; }

// Sweep 2 takes the fast path when no slot of the adjoint ring is touched twice within a chunk of C rows: every far read at least C
// rows old (its target is no row's own slot within the chunk), and any two reads of one far line at least C apart (no two rows share
// a target).  A line's depth is its deepest read, so every other read is then at most D - C: no target wraps onto a row's own slot
// either, and the read at the full depth finds the slot its own row just reset.
bool far_fast_path(const Graph& g, uint32_t C)
{
   const RingLayout rl = ring_layout(g);
   for (size_t i = 0; i < rl.far_reads.size(); ++i) {
      if (rl.far_reads[i].second < C) return false;
      for (size_t j = 0; j < i; ++j) {
         const uint32_t a = rl.far_reads[i].second, b = rl.far_reads[j].second;
         if (rl.far_reads[i].first == rl.far_reads[j].first && (a > b ? a - b : b - a) < C) return false;
      }
   }
   return true;
}

// struct fz_adj: fwd() -- the state after one step, from the state before it and the step's frame (the forward step() of gen_body for
// one stream per lane, outputs left out) -- and bwd() -- the same step re-evaluated, then the adjoint statements in reverse node order.
// The order of every sum is the one include/flowz_hip.h documents (fz_run_block_grad); tests/adjoint_ref.py restates it.  A node's
// adjoint starts as -0.0f, the identity of IEEE addition: a first contribution is the contribution itself, bit for bit, and the
// compiler folds the addition away.  Nodes no adjoint reaches (those that only feed comparisons) emit nothing at all.
// loss (FZ_VF_ADJOINT_LOSS): out() as well -- the step's output values from (x, c, p, s), for the kernels that form dL/dy themselves;
// without it the text is what it was before that variant existed, byte for byte.
// ring (FZ_VF_ADJOINT_RING, fz_kernel_adjoint_ring.hip.inc): the lines in LDS leave the register arrays -- s / sn / R hold the rows of
// the other lines, compact (ring_layout) --; a delayed read of such a line is rv[read], fwd() hands the lines' source values out in
// u[], and bwd() keeps their pending adjoints in the lane's LDS column `ring` (pt[line] = the row number modulo the line's depth):
// rule 2 reads the row's slot and resets it to -0.0f, the pending adjoints the step's reads add into are loaded together behind that
// (a read at the full depth finds the slot just reset), receive rule 3's additions in registers in its order and are stored once.
// Without it -- every ring-free graph -- the text is byte for byte what it was.
// loss and ring (fz_kernel_adjoint_ring.hip.inc with FZ_LOSS): out() takes rv as well -- a delayed read of a ring line is rv[read] there too.
// far (FZ_VF_ADJOINT_FAR, fz_kernel_adjoint_ring.hip.inc with FZ_FAR; always with ring): the lines in HBM are neither register rows nor LDS slots.
// A delayed read of one is rv[n ring reads + far read], fwd() hands its source value out in u[n ring lines + far line], and bwd()
// treats its pending adjoints as it treats a ring line's, in one of two places.  far == 1, the per-row path: the ring column is the
// global pointer `fa` with stride `ns` (row fz_fl_slot0 + slot of the workspace ring, fpt[far line] = the slot of the row) -- load,
// add, store in program order.  far == 2, the fast path: the kernel has requested the row's slots with the chunk's rows -- f2[far
// line] is rule 2's slot, fq[far read] comes in as the pending adjoint the read adds into (-0.0f at the full depth: the slot just
// reset) and goes out as what the kernel stores there.
std::string gen_adjoint_body(const Graph& g, bool loss, bool ring, int far)
{
   std::ostringstream o;
   const RingLayout rl = ring ? ring_layout(g) : RingLayout();
   auto far_line = [&](size_t line) { return far ? rl.far_of_line[line] : -1; };
   auto far_read_of = [&](const Node& nd) { return rl.far_read_index((uint32_t)far_line((size_t)g.line_of_node[nd.a]), nd.b); };
   auto far_slot = [&](int f, uint32_t d) {                // the workspace-ring row of far line f `d` rows back
      const uint32_t D = g.lines[rl.fl_line[(size_t)f]].depth, s0 = rl.fl_slot0[(size_t)f];
      const std::string pt = "fpt[" + std::to_string(f) + "]";
      const std::string q = d == 0 || d == D ? pt : "(" + pt + " >= " + std::to_string(d) + "u ? " + pt + " - " + std::to_string(d) + "u : " + pt + " + " + std::to_string(D - d) + "u)";
      return "fa[(size_t)(" + std::to_string(s0) + "u + " + q + ") * ns]";
   };
   // ring mode: the ring line a line is (-1: a register line), the ring read a DELAY node is, the slot of a ring line `d` rows back
   auto ring_line = [&](size_t line) { return ring ? rl.ring_of_line[line] : -1; };
   auto read_of = [&](const Node& nd) { return rl.read_index((uint32_t)ring_line((size_t)g.line_of_node[nd.a]), nd.b); };
   auto slot = [&](int k, uint32_t d) {
      const uint32_t D = g.lines[rl.rl_line[(size_t)k]].depth, s0 = rl.rl_slot0[(size_t)k];
      const std::string pt = "pt[" + std::to_string(k) + "]";
      const std::string q = d == 0 || d == D ? pt : "(" + pt + " >= " + std::to_string(d) + "u ? " + pt + " - " + std::to_string(d) + "u : " + pt + " + " + std::to_string(D - d) + "u)";
      return "ring[(size_t)(" + std::to_string(s0) + "u + " + q + ") * FZ_BLOCK]";
   };
   auto val = [&](uint32_t id) { return "v" + std::to_string(id); };
   auto adj = [&](uint32_t id) { return "g" + std::to_string(id); };
   o << "// generated by libflowz_hip -- adjoint graph body: " << g.nodes.size() << " nodes, " << g.lines.size() << " delay lines, " << g.n_state
     << " state floats\n";
   emit_functions(o, g, true);
   auto row = [&](uint32_t src, uint32_t age) {          // state row of node src's value `age` samples ago (age >= 1)
      const Line& L = g.lines[(size_t)g.line_of_node[src]];
      if (ring) return (uint32_t)rl.reg0[(size_t)g.line_of_node[src]] + age - 1;
      return L.row0 + age - 1;
   };
   auto values = [&](const char* indent) {
      for (size_t id = 0; id < g.nodes.size(); ++id) {
         const Node& nd = g.nodes[id];
         if (!adjoint_takes(nd.kind)) fail(FZ_E_UNSUPPORTED, "internal: a node kind the adjoint kernel does not take");
         o << indent << "const float " << val((uint32_t)id) << " = ";
         switch (nd.kind) {
            case FZ_IR_INPUT: o << "x[" << nd.a << "]"; break;
            case FZ_IR_CONST: o << "c[" << nd.a << "]"; break;
            case FZ_IR_PARAM: o << "p[" << nd.a << "]"; break;
            case FZ_IR_DELAY:
               if (ring_line((size_t)g.line_of_node[nd.a]) >= 0) o << "rv[" << read_of(nd) << "]";
               else if (far_line((size_t)g.line_of_node[nd.a]) >= 0) o << "rv[" << rl.n_rr() + (uint32_t)far_read_of(nd) << "]";
               else o << "s[" << row(nd.a, nd.b) << "]";
               break;
            default: o << op_expr(nd.kind, false, [&](uint32_t k, bool) { return val(operand(nd, k)); });
         }
         o << ";\n";
      }
   };
   o << "struct fz_adj {\n";
   o << "   // the state after one step: row (row0 + j) of a line holds its source's value j + 1 samples ago\n";
   if (ring) {
      o << "   // (s / sn: the rows of the lines in registers, compact; rv: the step's ring-read values; u: the ring lines' source values)\n";
      o << "   __device__ __forceinline__ static void fwd(const float* x, const float* c, const float* p, const float* s, const float* rv, float* sn,\n"
           "                                              float* u)\n   {\n";
      o << "      (void)x; (void)c; (void)p; (void)s; (void)rv; (void)sn; (void)u;\n";
   } else {
      o << "   __device__ __forceinline__ static void fwd(const float* x, const float* c, const float* p, const float* s, float* sn)\n   {\n";
      o << "      (void)x; (void)c; (void)p; (void)s; (void)sn;\n";
   }
   values("      ");
   for (size_t l = 0; l < g.lines.size(); ++l) {
      const Line& L = g.lines[l];
      if (ring_line(l) >= 0) {
         o << "      u[" << ring_line(l) << "] = " << val(L.src) << ";\n";
         continue;
      }
      if (far_line(l) >= 0) {
         o << "      u[" << rl.n_rl() + (uint32_t)far_line(l) << "] = " << val(L.src) << ";\n";
         continue;
      }
      const uint32_t r0 = ring ? (uint32_t)rl.reg0[l] : L.row0;
      o << "      sn[" << r0 << "] = " << val(L.src) << ";\n";
      for (uint32_t a = 1; a < L.depth; ++a) o << "      sn[" << r0 + a << "] = s[" << r0 + a - 1 << "];\n";
   }
   o << "   }\n";
   o << "   // one step backwards: yb = dL/dy of the step, R = the pending line adjoints (the state after the step on entry, before it on\n"
        "   // return), pb / cb += this step's parameter / coefficient adjoints, xb = dL/dx of the step\n";
   if (far) {
      o << "   // (ring, pt: the ring lines' pending adjoints in the lane's LDS column, the row number modulo each line's depth; the far lines':\n";
      o << (far == 2 ? "   //  f2[far line] = the slot of the row, fq[far read] = the pending adjoint the read adds into, in and out)\n"
                     : "   //  fa = the lane's column of the workspace ring, stride ns; fpt[far line] = the slot of the row)\n");
      o << "   __device__ __forceinline__ static void bwd(const float* x, const float* c, const float* p, const float* s, const float* rv, const float* yb,\n"
           "                                              float* xb, float* R, float* pb, float* cb, float* ring, const unsigned* pt, "
        << (far == 2 ? "const float* f2, float* fq" : "float* fa, const unsigned* fpt, size_t ns") << ")\n   {\n";
      o << "      (void)x; (void)c; (void)p; (void)s; (void)rv; (void)yb; (void)xb; (void)R; (void)pb; (void)cb; (void)ring; (void)pt; "
        << (far == 2 ? "(void)f2; (void)fq;" : "(void)fa; (void)fpt; (void)ns;") << "\n";
   } else if (ring) {
      o << "   // (ring: the lane's LDS column of the ring lines' pending adjoints; pt[line]: the row number modulo the line's depth)\n";
      o << "   __device__ __forceinline__ static void bwd(const float* x, const float* c, const float* p, const float* s, const float* rv, const float* yb,\n"
           "                                              float* xb, float* R, float* pb, float* cb, float* ring, const unsigned* pt)\n   {\n";
      o << "      (void)x; (void)c; (void)p; (void)s; (void)rv; (void)yb; (void)xb; (void)R; (void)pb; (void)cb; (void)ring; (void)pt;\n";
   } else {
      o << "   __device__ __forceinline__ static void bwd(const float* x, const float* c, const float* p, const float* s, const float* yb, float* xb,\n"
           "                                              float* R, float* pb, float* cb)\n   {\n";
      o << "      (void)x; (void)c; (void)p; (void)s; (void)yb; (void)xb; (void)R; (void)pb; (void)cb;\n";
   }
   values("      ");
   const size_t n = g.nodes.size();
   std::vector<char> has(n, 0);
   for (size_t id = 0; id < n; ++id) o << "      float " << adj((uint32_t)id) << " = -0.0f;\n";
   o << "      // 1. output slots, in slot order\n";
   for (size_t j = 0; j < g.outputs.size(); ++j) {
      o << "      " << adj(g.outputs[j]) << " = " << adj(g.outputs[j]) << " + yb[" << j << "];\n";
      has[g.outputs[j]] = 1;
   }
   o << "      // 2. the pending line adjoint: row row0 of the state after the step is the line source's value; the other rows move one up\n";
   for (size_t l = 0; l < g.lines.size(); ++l) {
      const Line& L = g.lines[l];
      has[L.src] = 1;
      if (ring_line(l) >= 0) {                             // (the ring does not move: the row's slot is read and becomes the deepest row's)
         o << "      " << adj(L.src) << " = " << adj(L.src) << " + " << slot(ring_line(l), 0) << ";\n";
         o << "      " << slot(ring_line(l), 0) << " = -0.0f;\n";
         continue;
      }
      if (far_line(l) >= 0) {                              // (fast path: the kernel resets the slot when it stores the row's slots)
         if (far == 2) o << "      " << adj(L.src) << " = " << adj(L.src) << " + f2[" << far_line(l) << "];\n";
         else {
            o << "      " << adj(L.src) << " = " << adj(L.src) << " + " << far_slot(far_line(l), 0) << ";\n";
            o << "      " << far_slot(far_line(l), 0) << " = -0.0f;\n";
         }
         continue;
      }
      const uint32_t r0 = ring ? (uint32_t)rl.reg0[l] : L.row0;
      o << "      " << adj(L.src) << " = " << adj(L.src) << " + R[" << r0 << "];\n";
      for (uint32_t a = 0; a + 1 < L.depth; ++a) o << "      R[" << r0 + a << "] = R[" << r0 + a + 1 << "];\n";
      o << "      R[" << r0 + L.depth - 1 << "] = -0.0f;\n";
   }
   if (ring) {
      o << "      // the pending adjoints the step's ring reads add into, loaded together (a read at the full depth: the slot just reset)\n";
      for (size_t i = 0; i < rl.reads.size(); ++i) {
         const uint32_t D = g.lines[rl.rl_line[rl.reads[i].first]].depth;
         o << "      float q" << i << "r = " << (rl.reads[i].second == D ? std::string("-0.0f") : slot((int)rl.reads[i].first, rl.reads[i].second)) << ";\n";
      }
   }
   if (far) {
      o << "      // the same for the far reads\n";
      for (size_t i = 0; i < rl.far_reads.size(); ++i) {
         const uint32_t D = g.lines[rl.fl_line[rl.far_reads[i].first]].depth;
         o << "      float qf" << i << "r = ";
         if (far == 2) o << "fq[" << i << "]";
         else o << (rl.far_reads[i].second == D ? std::string("-0.0f") : far_slot((int)rl.far_reads[i].first, rl.far_reads[i].second));
         o << ";\n";
      }
   }
   o << "      // 3. consumers in decreasing node order\n";
   auto plus = [&](uint32_t to, const std::string& e) {
      o << "      " << adj(to) << " = " << adj(to) << " + " << e << ";\n";
      has[to] = 1;
   };
   auto minus = [&](uint32_t to, const std::string& e) {
      o << "      " << adj(to) << " = " << adj(to) << " - " << e << ";\n";
      has[to] = 1;
   };
   for (size_t k = n; k-- > 0;) {
      const Node& nd = g.nodes[k];
      if (!has[k]) continue;
      const std::string gk = adj((uint32_t)k), va = val(nd.a), vb = val(nd.b), vk = val((uint32_t)k);
      switch (nd.kind) {
         case FZ_IR_INPUT: break;
         case FZ_IR_CONST: o << "      cb[" << nd.a << "] = cb[" << nd.a << "] + " << gk << ";\n"; break;
         case FZ_IR_PARAM: o << "      pb[" << nd.a << "] = pb[" << nd.a << "] + " << gk << ";\n"; break;
         case FZ_IR_DELAY: {
            if (ring_line((size_t)g.line_of_node[nd.a]) >= 0) {
               o << "      q" << read_of(nd) << "r = q" << read_of(nd) << "r + " << gk << ";\n";
               break;
            }
            if (far_line((size_t)g.line_of_node[nd.a]) >= 0) {
               o << "      qf" << far_read_of(nd) << "r = qf" << far_read_of(nd) << "r + " << gk << ";\n";
               break;
            }
            const uint32_t r = row(nd.a, nd.b);
            o << "      R[" << r << "] = R[" << r << "] + " << gk << ";\n";
            break;
         }
         case FZ_IR_ADD: plus(nd.a, gk); plus(nd.b, gk); break;
         case FZ_IR_SUB: plus(nd.a, gk); minus(nd.b, gk); break;
         case FZ_IR_MUL: plus(nd.a, gk + " * " + vb); plus(nd.b, gk + " * " + va); break;
         case FZ_IR_DIV:
            o << "      const float q" << k << " = " << gk << " / " << vb << ";\n";
            plus(nd.a, "q" + std::to_string(k));
            minus(nd.b, "q" + std::to_string(k) + " * " + vk);
            break;
         case FZ_IR_NEG: minus(nd.a, gk); break;
         case FZ_IR_SQRT: plus(nd.a, gk + " * (0.5f / " + vk + ")"); break;
         case FZ_IR_EXP: plus(nd.a, gk + " * " + vk); break;
         case FZ_IR_TANH: plus(nd.a, gk + " * (1.0f - " + vk + " * " + vk + ")"); break;
         case FZ_IR_SIN: plus(nd.a, gk + " * fz_cos(" + va + ")"); break;
         case FZ_IR_COS: minus(nd.a, gk + " * fz_sin(" + va + ")"); break;
         case FZ_IR_LOG: plus(nd.a, gk + " / " + va); break;
         case FZ_IR_ABS:
            o << "      " << adj(nd.a) << " = " << va << " > 0.f ? " << adj(nd.a) << " + " << gk << " : " << va << " < 0.f ? " << adj(nd.a) << " - " << gk
              << " : " << adj(nd.a) << ";\n";
            has[nd.a] = 1;
            break;
         case FZ_IR_MIN: case FZ_IR_MAX: {
            // all of g to the operand std::min / std::max returned: min = (b < a) ? b : a, max = (a < b) ? b : a
            const std::string m = "m" + std::to_string(k);
            o << "      const bool " << m << " = " << (nd.kind == FZ_IR_MIN ? vb + " < " + va : va + " < " + vb) << ";\n";
            o << "      " << adj(nd.a) << " = " << m << " ? " << adj(nd.a) << " : " << adj(nd.a) << " + " << gk << ";\n";
            o << "      " << adj(nd.b) << " = " << m << " ? " << adj(nd.b) << " + " << gk << " : " << adj(nd.b) << ";\n";
            has[nd.a] = has[nd.b] = 1;
            break;
         }
         default: break;                                   // comparisons: derivative zero, no arithmetic
      }
   }
   if (ring) {
      o << "      // the ring reads' pending adjoints back into their slots, once each\n";
      for (size_t i = 0; i < rl.reads.size(); ++i) o << "      " << slot((int)rl.reads[i].first, rl.reads[i].second) << " = q" << i << "r;\n";
   }
   for (size_t i = 0; far && i < rl.far_reads.size(); ++i) {
      if (far == 2) o << "      fq[" << i << "] = qf" << i << "r;\n";
      else o << "      " << far_slot((int)rl.far_reads[i].first, rl.far_reads[i].second) << " = qf" << i << "r;\n";
   }
   o << "      // 4. the step's input adjoints (+0 for a wire no adjoint reaches)\n";
   for (uint32_t w = 0; w < g.n_in; ++w) {
      std::string e = "0.0f";
      for (size_t id = 0; id < n; ++id)
         if (g.nodes[id].kind == FZ_IR_INPUT && g.nodes[id].a == w && has[id]) e = e == "0.0f" ? adj((uint32_t)id) : e + " + " + adj((uint32_t)id);
      o << "      xb[" << w << "] = " << e << ";\n";
   }
   o << "   }\n";
   if (loss) {
      o << "   // the step's output values, slot by slot: the bits fz_run_block writes\n";
      if (ring) {
         o << "   // (s: the rows of the lines in registers, compact; rv: the step's ring-read values)\n";
         o << "   __device__ __forceinline__ static void out(const float* x, const float* c, const float* p, const float* s, const float* rv, float* y)\n   {\n";
         o << "      (void)x; (void)c; (void)p; (void)s; (void)rv; (void)y;\n";
      } else {
         o << "   __device__ __forceinline__ static void out(const float* x, const float* c, const float* p, const float* s, float* y)\n   {\n";
         o << "      (void)x; (void)c; (void)p; (void)s; (void)y;\n";
      }
      values("      ");
      for (size_t j = 0; j < g.outputs.size(); ++j) o << "      y[" << j << "] = " << val(g.outputs[j]) << ";\n";
      o << "   }\n";
   }
   o << "};\n";
   return o.str();
}

}  // namespace fz
