// Kernel manifests.  FLOWZ_HIP_MANIFEST=<file>: every kernel a process resolves for the first time is appended as (recipe of its program,
// variant) -- a few hundred bytes.  fz_manifest_build replays such a file WITHOUT a GPU: compiles the programs again and builds, in parallel
// compiler processes, whatever the kernel cache lacks.  The records name expressions and variants, not generated text: a replay after the
// kernel skeleton or the code generator changed builds the NEW kernels of the same launches (round 5: the GPU test suite launches ~1800
// kernels; a box that has to JIT them all needs 10 minutes for what takes 80 s from a warm cache).
#include <fcntl.h>
#include <sys/file.h>
#include <unistd.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <thread>

#include "fz_runtime.hpp"

namespace fz {

void manifest_record(const fz_program* p, const Variant& v)
{
   static const char* const path = std::getenv("FLOWZ_HIP_MANIFEST");
   if (!path || !*path || p->recipe.empty()) return;
   char head[96];
   std::snprintf(head, sizeof head, "FZM1 %u %u %u %u %zu\n", v.P, v.U, v.block, v.flags, p->recipe.size());
   const std::string rec = head + p->recipe;
   {
      static std::mutex mu;
      static std::set<uint64_t> seen;                      // (a test suite compiles the same graphs hundreds of times)
      std::lock_guard<std::mutex> lock(mu);
      if (!seen.insert(fnv1a(rec)).second) return;
   }
   const int fd = ::open(path, O_WRONLY | O_CREAT | O_APPEND, 0644);
   if (fd < 0) return;
   (void)::flock(fd, LOCK_EX);                             // (several processes may share the file: records never interleave)
   size_t off = 0;
   while (off < rec.size()) {
      const ssize_t n = ::write(fd, rec.data() + off, rec.size() - off);
      if (n <= 0) break;
      off += (size_t)n;
   }
   (void)::flock(fd, LOCK_UN);
   ::close(fd);
}

// What a record's variant must satisfy before anything is generated from it: a forward kernel runs 1, 2 or 4 streams per lane.  A
// variant of the adjoint family has rules of its own and one home for them, fz_grad.cpp: grad_variant_fits -- asked below, once the
// record's graph is compiled; a PCM variant passes the forward rule and then fz_pcm16.cpp: pcm16_variant_fits, or pcm16_sm_variant_fits
// where it names the kernel for stream-major buffers.  The forward of far lines on stream-major buffers carries its patch rows in P and has
// one home for its rule as well, fz_far_sm.cpp: far_sm_variant_fits.
static bool variant_is_sane(const Variant& v)
{
   if ((v.flags & FZ_VF_ADJOINT) || is_far_sm(v.flags)) return true;
   return (v.P == 1 || v.P == 2 || v.P == 4) && v.U != 0 && v.U <= 128 && v.block != 0 && v.block % 64 == 0 && v.block <= 1024;
}

int manifest_build(const std::string& path, unsigned n_workers, uint32_t counts[4])
{
   const std::string text = slurp(path);
   if (text.empty()) fail(FZ_E_INVALID, "kernel manifest: cannot read " + path);
   // records -> unique (recipe, variant) pairs
   std::map<std::string, std::set<Variant>> want;
   size_t pos = 0;
   uint32_t bad_records = 0;
   while (pos < text.size()) {
      const size_t eol = text.find('\n', pos);
      if (eol == std::string::npos) break;
      Variant v;
      size_t n = 0;
      if (std::sscanf(text.c_str() + pos, "FZM1 %u %u %u %u %zu", &v.P, &v.U, &v.block, &v.flags, &n) != 5 || n > text.size() - (eol + 1))
         fail(FZ_E_INVALID, "kernel manifest: damaged record at byte " + std::to_string(pos));
      pos = eol + 1 + n;
      // (the file is data from elsewhere: a variant no launch could have resolved -- it would divide by P or size a workgroup by `block`
      //  further down -- is counted as failed, not built)
      if (!variant_is_sane(v)) {
         ++bad_records;
         continue;
      }
      want[text.substr(eol + 1, n)].insert(v);
   }
   struct Item { fz_program* p; Variant v; };
   std::vector<std::unique_ptr<fz_program>> programs;
   std::vector<Item> items;
   counts[0] = counts[3] = bad_records;                    // records, at hand, built, failed
   counts[1] = counts[2] = 0;
   for (const auto& kv : want) {
      const std::string& recipe = kv.first;
      const size_t eol = recipe.find('\n');
      unsigned typed = 0;
      if (eol == std::string::npos || std::sscanf(recipe.c_str(), "typed %u", &typed) != 1) fail(FZ_E_INVALID, "kernel manifest: damaged recipe");
      std::vector<uint32_t> dt;
      {
         std::istringstream is(recipe.substr(7, eol - 7));
         for (unsigned d; is >> d;) dt.push_back(d);
      }
      fz_expr* e = parse_expr(recipe.substr(eol + 1));
      fz_program* p = nullptr;
      const int rc = !e ? FZ_E_INVALID : typed ? fz_compile_typed(e, dt.empty() ? nullptr : dt.data(), (uint32_t)dt.size(), &p) : fz_compile(e, &p);
      fz_expr_release(e);
      counts[0] += (uint32_t)kv.second.size();
      if (rc != FZ_OK || !p) {                              // (a graph this build of the library no longer accepts)
         counts[3] += (uint32_t)kv.second.size();
         continue;
      }
      programs.emplace_back(p);
      for (const Variant& v : kv.second) {
         if ((v.flags & FZ_VF_ADJOINT) && !grad_variant_fits(p->g, v)) ++counts[3];   // (no variant a backward makes for this graph: its flag set, stride, workgroup, patch rows)
         else if ((v.flags & FZ_VF_PCM16) && !((v.flags & FZ_VF_PCM16_SM) ? pcm16_sm_variant_fits(p->g, v) : pcm16_variant_fits(p->g, v))) ++counts[3];   // (no variant fz_run_block_pcm16 makes, or a graph it refuses)
         else if (is_far_sm(v.flags) && !far_sm_variant_fits(p->g, v)) ++counts[3];   // (not the variant fz_run_block_far_stream_major makes for this graph)
         else items.push_back(Item{p, v});
      }
   }
   std::atomic<size_t> next{0};
   std::atomic<uint32_t> at_hand{0}, built{0}, failed{0};
   auto work = [&] {
      for (size_t i; (i = next.fetch_add(1)) < items.size();) {
         try {
            if (kernel_at_hand(items[i].p, items[i].v)) {
               ++at_hand;
               continue;
            }
            (void)get_kernel(items[i].p, items[i].v, nullptr, true);   // (builds in parallel: a compiler process per kernel)
            ++built;
         } catch (const Error&) {
            ++failed;                                       // (a variant the graph no longer allows, a kernel that no longer compiles)
         } catch (const std::exception&) {
            ++failed;                                       // (anything else a damaged record provokes: never std::terminate from a worker thread)
         }
      }
   };
   std::vector<std::thread> ths;
   for (unsigned t = 1; t < std::max(1u, n_workers); ++t) ths.emplace_back(work);
   work();
   for (std::thread& t : ths) t.join();
   counts[1] = at_hand;
   counts[2] = built;
   counts[3] += failed;
   return FZ_OK;
}

}  // namespace fz
