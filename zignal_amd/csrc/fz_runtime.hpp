// Internal to the runtime half of libflowz_hip (the files that talk to HIP / hiprtc):
//   fz_rtc.cpp           which hiprtc compiles the kernels, in this process or in fz_rtc_worker; the build options
//   fz_kernel_cache.cpp  a kernel's key, the on-disk code-object cache, get_kernel, module loading, a code object's resources
//   fz_manifest.cpp      kernel manifests: record what a process resolves, replay it into the kernel cache
//   fz_plan.cpp          variant resolution: the library's static choice per layout and kernel body
//   fz_tune.cpp          measured plans: tune candidates, fz_program_tune, persistence per board
//   fz_launch.cpp        the launch of the fused block kernel; the one hipModuleLaunchKernel (its image: fz_kernargs.hpp)
//   fz_bank.cpp          device-resident closure state (fz_bank) and the host-frames pipelines
//   fz_aot_kernels.hip   the AOT utility kernels (synthetic fill, copy probe, RBJ coefficients, layout adapter)
#pragma once

#include <hip/hip_runtime_api.h>

#include <string>

#include "fz_internal.hpp"
#include "fz_kernargs.hpp"

namespace fz {

#define FZ_HIP(call)                                                                            \
   do {                                                                                         \
      hipError_t e_ = (call);                                                                   \
      if (e_ != hipSuccess)                                                                     \
         fail(FZ_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_));                     \
   } while (0)

void require_device();                       // FZ_E_NO_DEVICE: there is no CPU fallback in the product path
std::string cache_dir();                     // where code objects and plans.txt live ("" = nowhere)
std::string library_dir();                   // where libflowz_hip.so and fz_rtc_worker are installed
std::string slurp(const std::string& path);  // a file's bytes ("" = unreadable)
const std::string& preferred_identity();     // fz_rtc.cpp: the ROCm installation's hiprtc, what pre-built objects are named after
const std::string& compiler_identity();      // the hiprtc that builds for this process (each a part of the cache keys)
std::vector<const char*> build_options(const Graph& g, const Variant& v);
std::vector<char> compile_kernel(const Graph& g, const Variant& v, bool in_own_process);
void manifest_record(const fz_program* p, const Variant& v);   // fz_manifest.cpp: FLOWZ_HIP_MANIFEST
// fz_launch.cpp: the coefficient tails of p's graph into a kernarg image made for their counts, read under p->mu; and the one
// hipModuleLaunchKernel of the library -- fn (hipFunction_t) on `grid` workgroups of `threads` lanes, the image as its arguments
void copy_coefficients(KernArgs& ka, fz_program* p);
void launch_kernel(void* fn, unsigned grid, unsigned threads, void* stream, KernArgs& ka);

inline uint64_t fnv1a_bytes(const char* d, size_t n, uint64_t h = 1469598103934665603ull)
{
   for (size_t i = 0; i < n; ++i) h = (h ^ (unsigned char)d[i]) * 1099511628211ull;
   return h;
}
inline uint64_t fnv1a(const std::string& s, uint64_t h = 1469598103934665603ull) { return fnv1a_bytes(s.data(), s.size(), h); }

}  // namespace fz
