// The inspection calls of a kernel -- resources, symbol, source -- stated once for the files that export them (fz_grad.cpp: the adjoint
// family, fz_far_sm.cpp: the forward of far lines on stream-major buffers).  Kept out of fz_internal.hpp: the macro emits extern "C"
// functions.
#pragma once

#include "fz_internal.hpp"

namespace fz {
// the inspection calls of a kernel that one maker's Variant names, given that maker: resources (`fn` names the call in the refusal;
// `unroll` = the Variant's U), symbol, source
template <class Maker>
int inspect_resources(fz_program* p, fz_kernel_resources* out, const char* fn, Maker make)
{
   FZ_GUARD(
      if (!p || !out) fail(FZ_E_INVALID, std::string(fn) + ": bad arguments");
      *out = resources_of(p, make());
      return FZ_OK;)
}

template <class Maker>
long inspect_symbol(fz_program* p, char* buf, size_t cap, Maker make)
{
   return string_result(buf, cap, [&] {
      if (!p) fail(FZ_E_INVALID, "null program");
      return kernel_symbol(p->g, make());
   });
}

template <class Maker>
long inspect_source(fz_program* p, char* buf, size_t cap, Maker make)
{
   return string_result(buf, cap, [&] {
      if (!p) fail(FZ_E_INVALID, "null program");
      return full_source(p->g, make());
   });
}
}  // namespace fz

// The inspection calls of one kernel -- fz_program_<stem>_resources<suf>, fz_program_<stem>_kernel_symbol<suf> and
// fz_program_<stem>_source<suf> (include/flowz_hip.h declares each) -- from one statement of its Variant.  `who` names the resources
// call in its refusal; ARGS is what the calls take between the program and their results, every argument with its comma.
#define FZ_INSPECTION(stem, suf, who, ARGS, VARIANT)                                                                         \
   int fz_program_##stem##_resources##suf(fz_program* p, ARGS fz_kernel_resources* out)                                      \
   {                                                                                                                         \
      return fz::inspect_resources(p, out, who, [&] { return VARIANT; });                                                    \
   }                                                                                                                         \
   long fz_program_##stem##_kernel_symbol##suf(fz_program* p, ARGS char* buf, size_t cap)                                    \
   {                                                                                                                         \
      return fz::inspect_symbol(p, buf, cap, [&] { return VARIANT; });                                                       \
   }                                                                                                                         \
   long fz_program_##stem##_source##suf(fz_program* p, ARGS char* buf, size_t cap)                                           \
   {                                                                                                                         \
      return fz::inspect_source(p, buf, cap, [&] { return VARIANT; });                                                       \
   }
