// The backward of a block (include/flowz_hip.h: fz_run_block_grad): what the adjoint kernel supports, its checkpoint stride and
// workspace, argument checks and the launch.  The kernel text is fz_kernel_adjoint.hip.inc plus gen_adjoint_body (fz_codegen.cpp);
// its code objects go through the kernel cache as a Variant with FZ_VF_ADJOINT.
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "fz_runtime.hpp"

namespace fz {

constexpr uint32_t kGradBlock = 256;          // lanes (= streams) per workgroup of the adjoint kernel
constexpr uint32_t kGradMaxCheckpoint = 32;   // the chunk is unrolled: every step's state and frame stay in registers

std::string grad_unsupported_reason(const Graph& g)
{
   if (g.typed) return "typed programs (fz_compile_typed) are not supported by the backward";
   if (g.n_mod) return "sample-rate modulators (fz_modulator) are not supported by the backward";
   for (uint8_t part : g.out_part)
      if (part) return "complex wires are not supported by the backward";
   for (const Line& L : g.lines) {
      if (L.far) return "delay lines deeper than 256 samples (rings in HBM) are not supported by the backward";
      if (L.in_lds) return "delay lines deeper than 8 samples (rings in LDS) are not supported by the backward";
      if (L.part || L.f64) return "complex or double delay lines are not supported by the backward";
   }
   if (g.n_lds_slots || g.max_delay > kRegMaxDepth) return "delay lines deeper than 8 samples are not supported by the backward";
   for (const Node& nd : g.nodes) {
      if (nd.f64) return "float64 nodes (a C++ double literal, fz_literal_f64) are not supported by the backward";
      if (nd.kind == FZ_IR_MOD) return "sample-rate modulators (fz_modulator) are not supported by the backward";
      if (!adjoint_takes(nd.kind)) return "IR node kind " + std::to_string(nd.kind) + " (complex arithmetic) is not supported by the backward";
   }
   return "";
}

// The chunk of sweep 2 keeps C steps of state and frame in registers, (n_state + n_in) * C floats, next to one step's node values
// and the accumulators: at most 64 saved floats, 16 rows at most (measured: no graph of tests/test_grad_host.py spills).
uint32_t grad_default_checkpoint(const Graph& g)
{
   const uint32_t per_row = std::max<uint32_t>(g.n_state + g.n_in, 1);
   uint32_t C = 16;
   while (C > 1 && C * per_row > 64) C /= 2;
   return C;
}

static uint32_t checkpoint_of(const Graph& g, uint32_t checkpoint_rows)
{
   if (checkpoint_rows == 0) return grad_default_checkpoint(g);
   if (checkpoint_rows > kGradMaxCheckpoint || (checkpoint_rows & (checkpoint_rows - 1)))
      fail(FZ_E_INVALID, "checkpoint_rows must be 0 (library default) or a power of two <= 32");
   return checkpoint_rows;
}

static void require_supported(const Graph& g)
{
   const std::string why = grad_unsupported_reason(g);
   if (!why.empty()) fail(FZ_E_UNSUPPORTED, why);
}

static Variant adjoint_variant(const Graph& g, uint32_t checkpoint_rows)
{
   require_supported(g);
   Variant v;
   v.P = 1;
   v.U = checkpoint_of(g, checkpoint_rows);
   v.block = kGradBlock;
   v.flags = FZ_VF_ADJOINT;
   return v;
}

static uint64_t workspace_bytes(const Graph& g, uint64_t n_streams, uint32_t n_samples, uint32_t C)
{
   const uint64_t chunks = ((uint64_t)n_samples + C - 1) / C;
   return chunks * g.n_state * n_streams * 4u;
}

// kernarg image of `struct fz_adj_args` (fz_kernel_adjoint.hip.inc) up to the coefficient tail
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

static int run_grad(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t n_samples, void* stream)
{
   if (!p) fail(FZ_E_INVALID, "null program");
   if (!a) fail(FZ_E_INVALID, "fz_run_block_grad: null arguments");
   if (a->struct_size != sizeof(fz_grad_args))
      fail(FZ_E_INVALID, "fz_grad_args.struct_size is " + std::to_string(a->struct_size) + ", this library knows " + std::to_string(sizeof(fz_grad_args)));
   const Graph& g = p->g;
   const Variant v = adjoint_variant(g, a->checkpoint_rows);
   if (n_streams == 0 || n_samples == 0) return FZ_OK;     // an empty block: nothing to differentiate, nothing touched
   if (n_samples == 0xFFFFFFFFu) fail(FZ_E_INVALID, "n_samples must be below 2^32 - 1");
   if (n_streams >= (1ull << 30)) fail(FZ_E_UNSUPPORTED, "2^30 streams or more per launch: shard the streams");
   if (g.n_in && !a->in) fail(FZ_E_INVALID, "in is null but the graph has input wires");
   if (g.n_state && !a->state) fail(FZ_E_INVALID, "state is null but the graph has delay lines");
   if (g.n_param && !a->params) fail(FZ_E_INVALID, "params is null but the graph has per-stream coefficients");
   if (g.n_out && !a->out_grad) fail(FZ_E_INVALID, "out_grad is null but the graph has output wires");
   const uint64_t need = workspace_bytes(g, n_streams, n_samples, v.U);
   if (need && !a->workspace) fail(FZ_E_INVALID, "workspace is null: fz_program_grad_workspace says " + std::to_string(need) + " bytes");
   if (need && a->workspace_bytes < need)
      fail(FZ_E_INVALID, "workspace_bytes " + std::to_string(a->workspace_bytes) + " is less than the " + std::to_string(need) + " bytes fz_program_grad_workspace asks for");
   const uint64_t fr = (uint64_t)n_samples * n_streams * 4u, row = n_streams * 4u;
   struct Buf {
      const void* ptr;
      uint64_t bytes;
      const char* name;
      bool out;
   };
   // (only what the kernel touches: buffers of zero rows are never dereferenced)
   const std::vector<Buf> bufs = {
      {a->in, g.n_in ? fr * g.n_in : 0, "in", false},          {a->state, row * g.n_state, "state", false},
      {a->params, row * g.n_param, "params", false},           {a->out_grad, g.n_out ? fr * g.n_out : 0, "out_grad", false},
      {a->state_grad, row * g.n_state, "state_grad", false},   {a->in_grad, g.n_in ? fr * g.n_in : 0, "in_grad", true},
      {a->state0_grad, row * g.n_state, "state0_grad", true},  {a->param_grad, row * g.n_param, "param_grad", true},
      {a->const_grad, row * g.consts.size(), "const_grad", true}, {a->workspace, need, "workspace", true},
   };
   for (const Buf& b : bufs)
      if (b.ptr && (reinterpret_cast<uintptr_t>(b.ptr) & 15u)) fail(FZ_E_INVALID, std::string(b.name) + ": device pointers must be 16-byte aligned");
   for (size_t i = 0; i < bufs.size(); ++i)
      for (size_t j = i + 1; j < bufs.size(); ++j) {
         const Buf &x = bufs[i], &y = bufs[j];
         if (!(x.out || y.out) || !x.ptr || !y.ptr || !x.bytes || !y.bytes) continue;
         if (x.ptr == a->state_grad && y.ptr == a->state0_grad && x.ptr == y.ptr) continue;   // (sbar0 may overwrite sbar_T in place)
         const uintptr_t x0 = reinterpret_cast<uintptr_t>(x.ptr), y0 = reinterpret_cast<uintptr_t>(y.ptr);
         if (x0 < y0 + y.bytes && y0 < x0 + x.bytes) fail(FZ_E_INVALID, std::string(x.name) + " and " + y.name + " overlap");
      }
   require_device();
   void* fn = nullptr;
   (void)get_kernel(p, v, &fn);
   // (the size of the kernel's argument struct: 8-byte aligned -- a buffer of another size does not launch that struct)
   const size_t kbytes = (sizeof(AdjArgsHeader) + sizeof(float) * std::max<size_t>(g.consts.size(), 1) + 7) & ~size_t(7);
   std::vector<char> kbuf(kbytes, 0);
   const AdjArgsHeader h{a->in,      a->state,       a->params,     a->out_grad, a->state_grad, a->in_grad,
                         a->state0_grad, a->param_grad, a->const_grad, static_cast<float*>(a->workspace), (unsigned long long)n_streams, n_samples,
                         (unsigned int)((n_samples + (uint64_t)v.U - 1) / v.U)};
   std::memcpy(kbuf.data(), &h, sizeof h);
   {
      std::lock_guard<std::mutex> lock(p->mu);
      if (!g.consts.empty()) std::memcpy(kbuf.data() + sizeof h, g.consts.data(), sizeof(float) * g.consts.size());
   }
   size_t size = kbytes;
   void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, kbuf.data(), HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
   const unsigned grid = (unsigned)((n_streams + v.block - 1) / v.block);
   FZ_HIP(hipModuleLaunchKernel((hipFunction_t)fn, grid, 1, 1, v.block, 1, 1, 0, (hipStream_t)stream, nullptr, extra));
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

int fz_program_grad_resources(fz_program* p, uint32_t checkpoint_rows, fz_kernel_resources* out)
{
   FZ_GUARD(
      if (!p || !out) fail(FZ_E_INVALID, "fz_program_grad_resources: bad arguments");
      const Variant v = adjoint_variant(p->g, checkpoint_rows);
      const auto k = get_kernel(p, v, nullptr);
      *out = fz_kernel_resources{k->res.vgprs, k->res.agprs, k->res.sgprs, k->res.scratch_bytes, k->res.lds_bytes, k->res.vgpr_spills,
                                 k->res.sgpr_spills, v.U};
      return FZ_OK;)
}

long fz_program_grad_kernel_symbol(fz_program* p, uint32_t checkpoint_rows, char* buf, size_t cap)
{
   try {
      if (!p) fail(FZ_E_INVALID, "null program");
      const std::string s = kernel_symbol(p->g, adjoint_variant(p->g, checkpoint_rows));
      if (buf && cap) {
         const size_t n = std::min(cap - 1, s.size());
         std::memcpy(buf, s.data(), n);
         buf[n] = 0;
      }
      return (long)s.size();
   } catch (const fz::Error& er) {
      set_error(er.msg);
      return er.code;
   }
}

int fz_run_block_grad(fz_program* p, const fz_grad_args* a, uint64_t n_streams, uint32_t n_samples, void* hip_stream)
{
   FZ_GUARD(return run_grad(p, a, n_streams, n_samples, hip_stream);)
}

}  // extern "C"
