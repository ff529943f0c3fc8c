// Which hiprtc compiles the kernels, with which options, in this process or in fz_rtc_worker.  gfx950 only.
#include <hip/hiprtc.h>

#include <dlfcn.h>
#include <fcntl.h>
#include <limits.h>
#include <link.h>
#include <spawn.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

#include "fz_runtime.hpp"

extern char** environ;

namespace fz {

std::vector<const char*> build_options(const Graph& g, const Variant& v)
{
   // -ffp-contract=off: one rounding per graph node (no v_fma/v_fmac); IEEE division.
   // The SLP vectoriser is off: with one stream per lane it pairs unrelated scalar
   // mul/add into v_pk_* at the price of v_mov shuffles, a net VALU loss on gfx950.
   std::vector<const char*> o = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                                 "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize"};
   // The parts of a wave split carry ONE or two packed pairs of segments: so little instruction-level parallelism that the default
   // scheduler (which orders for occupancy) leaves dependent v_pk_mul / v_pk_add back to back -- two s_nop per step in the ISA on
   // top of the wait.  The max-ILP strategy interleaves the atoms: 411 instead of 477 instructions per round of 32 steps, no
   // s_nop; measured +9 % at 16 384 streams and +1-4 % at 32 768 with rounds of 32 steps (profiles/r03/sweep_sched_strategy.txt).
   // Rounds of 16 steps next to an I/O wave LOSE 15-20 % with it, and the single-wave kernels (three pairs: enough ILP) 0-4 %.
   if (ws_parts(v.flags) >= 2 && v.U == 32) {
      o.push_back("-mllvm");
      o.push_back("-amdgpu-sched-strategy=max-ilp");
   }
   // The pair long-run stream-major body (two streams per lane, ONE wave per SIMD): the graph of a step is one serial chain of packed
   // operations and nothing else shares the SIMD, so the default order (a step after the other: every v_pk_add behind the v_pk_mul
   // it waits for, 857 s_nop in the cascade's code) would run at the latency of the chain.  The iterative ILP scheduler overlaps
   // the stages of consecutive steps (286 s_nop, two to three chains in flight).
   // (deep graphs only: on shallow ones it hoists every LDS read of the unrolled steps and runs out of registers)
   if ((v.flags & FZ_VF_STREAM_MAJOR) && (v.flags & FZ_VF_SM_LONG) && v.P == 2 && sm_deep(g)) {
      o.push_back("-mllvm");
      o.push_back("-amdgpu-sched-strategy=iterative-ilp");
   }
   // developer hook (kernel experiments: -DFZ_DBG_NOLOAD ... and compiler flags); part of the cache key like every option
   static const std::vector<std::string> extra = [] {
      std::vector<std::string> e;
      if (const char* env = std::getenv("FLOWZ_HIP_EXTRA_OPTS")) {
         std::istringstream is(env);
         for (std::string t; is >> t;) e.push_back(t);
      }
      return e;
   }();
   for (const std::string& e : extra) o.push_back(e.c_str());
   return o;
}

// ---- which hiprtc compiles the kernels ----------------------------------------------------------------------------------
// The library links libhiprtc.so.7 of the ROCm installation it was built against.  A host process that has ANOTHER copy with that
// soname loaded already -- a PyTorch wheel bundles the ROCm release it was built with, hiprtc and comgr (the compiler) included --
// binds us to that copy instead, and the code would then depend on who imported what first: the wheel's older compiler needs 22 more
// registers for the four-streams-per-lane headline kernel, which therefore "has scratch" and the library steps down to two
// (0.73 instead of 0.77 of peak).  Round 4 closes that: a library that finds itself bound to a foreign hiprtc hands every build
// to fz_rtc_worker (fz_rtc_worker.cpp, installed next to the library): a fresh process whose only hiprtc is the installation's.
// Same compiler, same options, same text: the code objects are byte-identical to what a process without torch builds, and they
// are cached under the installation's name.  Only when the worker cannot be run (not installed, not executable, bound to
// something else itself) does the host process's compiler build the kernel -- under a cache name of its own, never standing in
// for the installation's, and with ONE warning on stderr (FLOWZ_HIP_QUIET=1 silences it).
// (Round 3 tried the same with dlmopen -- the installation's hiprtc in a link-map namespace of its own inside the host process;
//  one of five full test runs ended in a segmentation fault nobody could explain.  A process boundary has no such failure mode.)
#ifndef FZ_ROCM_LIB_DIR
#define FZ_ROCM_LIB_DIR "/opt/rocm/lib"
#endif
struct Rtc {
   std::string identity;                               // part of every cache key
   std::string worker;                                 // "" : in-process; else the fz_rtc_worker executable
};

static std::string real_path(const std::string& p)
{
   char buf[PATH_MAX];
   return ::realpath(p.c_str(), buf) ? std::string(buf) : p;
}

static std::string installed_hiprtc() { return real_path(std::string(FZ_ROCM_LIB_DIR) + "/libhiprtc.so.7"); }

// the identity of the installation's compiler: "libhiprtc.so.7.2.70200"
const std::string& preferred_identity()
{
   static const std::string id = [] {
      const std::string ours = installed_hiprtc();
      const size_t s = ours.rfind('/');
      return s == std::string::npos ? ours : ours.substr(s + 1);
   }();
   return id;
}

static std::string worker_path() { return library_dir() + "/fz_rtc_worker"; }

// run the worker: argv = {worker, request, output}; environment without LD_LIBRARY_PATH / LD_PRELOAD; its stdout goes to out_path
static int run_worker(const std::string& worker, const std::string& request, const std::string& output, const std::string& stdout_path)
{
   std::vector<std::string> envs;
   for (char** e = environ; e && *e; ++e)
      if (std::strncmp(*e, "LD_LIBRARY_PATH=", 16) != 0 && std::strncmp(*e, "LD_PRELOAD=", 11) != 0) envs.push_back(*e);
   std::vector<char*> envp;
   for (std::string& e : envs) envp.push_back(&e[0]);
   envp.push_back(nullptr);
   std::string a0 = worker, a1 = request, a2 = output;
   char* argv[] = {&a0[0], &a1[0], output.empty() ? nullptr : &a2[0], nullptr};
   posix_spawn_file_actions_t fa;
   posix_spawn_file_actions_init(&fa);
   posix_spawn_file_actions_addopen(&fa, 1, stdout_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0600);
   pid_t pid = 0;
   const int rc = posix_spawn(&pid, worker.c_str(), &fa, nullptr, argv, envp.data());
   posix_spawn_file_actions_destroy(&fa);
   if (rc != 0) return -1;
   int status = 0;
   while (waitpid(pid, &status, 0) < 0)
      if (errno != EINTR) return -1;
   return WIFEXITED(status) ? WEXITSTATUS(status) : -1;
}

std::string slurp(const std::string& path)
{
   std::ifstream f(path, std::ios::binary);
   return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// a private scratch directory for the worker's request / output files; gone, with those files, when the scope ends
struct WorkerDir {
   std::string dir;                                    // "" : there is no temporary directory
   WorkerDir()
   {
      const char* t = std::getenv("TMPDIR");
      dir = std::string(t && *t ? t : "/tmp") + "/fz_rtc_XXXXXX";
      if (!::mkdtemp(&dir[0])) dir.clear();
   }
   ~WorkerDir()
   {
      if (dir.empty()) return;
      for (const char* n : {"request", "code", "code.log", "stdout"}) ::unlink(file(n).c_str());
      ::rmdir(dir.c_str());
   }
   std::string file(const char* name) const { return dir + "/" + name; }
};

// why the worker cannot stand in for a foreign hiprtc ("" = it can): it must exist, run, and be bound to the installation's hiprtc itself
static std::string worker_refusal(const std::string& w, const std::string& ours)
{
   if (::access(w.c_str(), X_OK) != 0) (void)::chmod(w.c_str(), 0755);   // (a snapshot that dropped the mode bits)
   if (::access(w.c_str(), X_OK) != 0) return w + " is missing or not executable";
   const WorkerDir d;
   if (d.dir.empty()) return "no temporary directory";
   const int rc = run_worker(w, "--identify", "", d.file("stdout"));
   const std::string said = slurp(d.file("stdout"));
   if (rc != 0 || said.rfind("hiprtc ", 0) != 0) return "the worker did not start (exit " + std::to_string(rc) + ")";
   const std::string its = said.substr(7, said.find('\n') - 7);
   return real_path(its) != ours ? "the worker is bound to " + its : "";
}

// hiprtc loads the compiler itself (libamd_comgr) at its first build, by soname: a process that is bound to the installation's hiprtc but has
// loaded ANOTHER comgr by then (the library imported first, a PyTorch wheel -- with the comgr it bundles -- after it, the first kernel built
// after that) would compile with the wheel's older compiler under the installation's name.  So every in-process build until the first one
// that found no foreign comgr (from then on hiprtc holds the installation's) asks: is a comgr loaded that is not the installation's?  If so
// that build goes to the worker, like the builds of a process bound to a foreign hiprtc.  Nothing is loaded on the host process's behalf.
static bool foreign_comgr_loaded()
{
   const std::string ours = real_path(std::string(FZ_ROCM_LIB_DIR) + "/libamd_comgr.so");
   struct Ctx { const std::string* ours; bool foreign; } ctx{&ours, false};
   dl_iterate_phdr([](struct dl_phdr_info* i, size_t, void* c) {
      Ctx& x = *static_cast<Ctx*>(c);
      if (i->dlpi_name && std::strstr(i->dlpi_name, "libamd_comgr") && real_path(i->dlpi_name) != *x.ours) x.foreign = true;
      return 0;
   }, &ctx);
   return ctx.foreign;
}

static const Rtc& rtc()
{
   static const Rtc r = [] {
      Rtc t;
      Dl_info info;
      const std::string bound = dladdr((const void*)&hiprtcCompileProgram, &info) && info.dli_fname ? real_path(info.dli_fname) : std::string("?");
      const std::string ours = installed_hiprtc();
      bool foreign = bound != ours && ::access(ours.c_str(), R_OK) == 0;
      std::string why;
      if (foreign && (why = worker_refusal(worker_path(), ours)).empty()) {
         t.worker = worker_path();
         foreign = false;
      }
      // identity: the installation's hiprtc by its versioned file name (computable without loading it: see preferred_identity),
      // any other by path and size
      struct stat st;
      t.identity = foreign ? "foreign:" + bound + ":" + std::to_string(::stat(bound.c_str(), &st) == 0 ? (long long)st.st_size : -1LL) : preferred_identity();
      if (foreign && !std::getenv("FLOWZ_HIP_QUIET"))
         std::fprintf(stderr, "[flowz_hip] warning: kernels that are not in the cache will be built by %s, the hiprtc the host process loaded first, not by the "
                              "ROCm installation's (%s): %s.  Such kernels may need more registers (a spilling variant steps down to a slower one); "
                              "objects pre-built by the installation's compiler are still preferred.\n", bound.c_str(), ours.c_str(), why.c_str());
      if (std::getenv("FLOWZ_HIP_DEBUG"))
         std::fprintf(stderr, "[flowz_hip] kernels are built by %s%s\n", (t.worker.empty() ? bound : ours).c_str(), t.worker.empty() ? "" : " in a process of its own (fz_rtc_worker: the host process is bound to another hiprtc)");
      return t;
   }();
   return r;
}

const std::string& compiler_identity() { return rtc().identity; }

static std::vector<char> jit_compile_in_process(const std::string& skel, const std::string& cfg, const std::string& body, const std::vector<const char*>& opts)
{
   const char* headers[2] = {cfg.c_str(), body.c_str()};
   const char* names[2] = {"fz_graph_config.h", "fz_graph_body.h"};
   hiprtcProgram prog;
   if (hiprtcCreateProgram(&prog, skel.c_str(), "fz_block_kernel.hip", 2, headers, names) != HIPRTC_SUCCESS)
      fail(FZ_E_COMPILE, "hiprtcCreateProgram failed");
   hiprtcResult r = hiprtcCompileProgram(prog, (int)opts.size(), const_cast<const char**>(opts.data()));
   if (r != HIPRTC_SUCCESS) {
      size_t n = 0;
      hiprtcGetProgramLogSize(prog, &n);
      std::string log(n, ' ');
      if (n) hiprtcGetProgramLog(prog, &log[0]);
      hiprtcDestroyProgram(&prog);
      fail(FZ_E_COMPILE, std::string("hiprtc: ") + hiprtcGetErrorString(r) + "\n" + log);
   }
   size_t n = 0;
   hiprtcGetCodeSize(prog, &n);
   std::vector<char> code(n);
   hiprtcGetCode(prog, code.data());
   hiprtcDestroyProgram(&prog);
   return code;
}

static std::vector<char> jit_compile_in_worker(const std::string& worker, const std::string& skel, const std::string& cfg, const std::string& body, const std::vector<const char*>& opts)
{
   const WorkerDir d;
   if (d.dir.empty()) fail(FZ_E_COMPILE, "fz_rtc_worker: no temporary directory for the request");
   {
      std::ofstream f(d.file("request"), std::ios::binary);
      auto section = [&](const char* kind, const char* name, const std::string& data) {
         f << kind << ' ' << name << ' ' << data.size() << '\n';
         f.write(data.data(), (std::streamsize)data.size());
         f << '\n';
      };
      f << "FZRTC1 " << (3 + opts.size()) << '\n';
      section("source", "fz_block_kernel.hip", skel);
      section("header", "fz_graph_config.h", cfg);
      section("header", "fz_graph_body.h", body);
      for (const char* o : opts) section("option", "-", o);
   }
   const int rc = run_worker(worker, d.file("request"), d.file("code"), d.file("stdout"));
   if (rc == 3) fail(FZ_E_COMPILE, slurp(d.file("code.log")));
   const std::string bytes = rc == 0 ? slurp(d.file("code")) : std::string();
   if (rc != 0 || bytes.size() < 64) fail(FZ_E_COMPILE, "fz_rtc_worker failed (exit " + std::to_string(rc) + ")");
   return std::vector<char>(bytes.begin(), bytes.end());
}

// in_own_process: a compiler process per build even where this process's hiprtc is the installation's (manifest builds compile in
// parallel: every thread hands its kernels to a compiler process of its own)
std::vector<char> compile_kernel(const Graph& g, const Variant& v, bool in_own_process)
{
   const std::string cfg = gen_config(g, v), body = gen_body(g, v);
   const std::vector<const char*> opts = build_options(g, v);
   std::string worker = rtc().worker;
   if (worker.empty() && in_own_process && compiler_identity() == preferred_identity() && ::access(worker_path().c_str(), X_OK) == 0) worker = worker_path();
   const std::string& skel = skeleton_source(v);
   if (!worker.empty()) return jit_compile_in_worker(worker, skel, cfg, body, opts);
   static std::mutex in_process;                          // (hiprtc in one process: one build at a time)
   std::lock_guard<std::mutex> lock(in_process);
   static bool comgr_is_ours = false;                     // (an in-process build has run with no foreign comgr around: hiprtc holds the installation's)
   if (!comgr_is_ours && compiler_identity() == preferred_identity()) {
      if (foreign_comgr_loaded() && ::access(worker_path().c_str(), X_OK) == 0) return jit_compile_in_worker(worker_path(), skel, cfg, body, opts);
      std::vector<char> code = jit_compile_in_process(skel, cfg, body, opts);
      comgr_is_ours = !foreign_comgr_loaded();
      return code;
   }
   return jit_compile_in_process(skel, cfg, body, opts);
}

}  // namespace fz
