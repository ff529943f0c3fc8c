// The kernel cache: a variant's key, the on-disk code-object cache and its one lookup, get_kernel (look up, else build and store),
// module loading and unloading, and what a code object's notes say the kernel needs.  gfx950 only.
#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "fz_runtime.hpp"

namespace fz {

int device_count()
{
   int n = 0;
   if (hipGetDeviceCount(&n) != hipSuccess) {
      (void)hipGetLastError();
      return 0;
   }
   return n;
}

void require_device()
{
   if (device_count() <= 0)
      fail(FZ_E_NO_DEVICE, "no HIP device visible: libflowz_hip evaluates flow-graphs on an MI355X only "
                           "(there is no CPU fallback in the product path)");
}

Kernel::~Kernel()
{
   if (loaded.empty()) return;
   int cur = 0;
   (void)hipGetDevice(&cur);
   for (const Loaded& l : loaded) {
      (void)hipSetDevice(l.device);
      (void)hipDeviceSynchronize();          // launches are asynchronous: never unload code that may still run
      (void)hipModuleUnload((hipModule_t)l.module);
   }
   (void)hipSetDevice(cur);
}

void* Kernel::function_on_current_device(const std::string& symbol)
{
   int dev = 0;
   FZ_HIP(hipGetDevice(&dev));
   for (const Loaded& l : loaded)
      if (l.device == dev) return l.function;
   hipModule_t mod;
   FZ_HIP(hipModuleLoadData(&mod, code.data()));
   hipFunction_t fn;
   FZ_HIP(hipModuleGetFunction(&fn, mod, symbol.c_str()));
   loaded.push_back(Loaded{dev, mod, fn});
   return fn;
}

// ---- where code objects are cached ----------------------------------------------------------------------------------
// the directory `up` levels above the library's file (.../zignal_amd/lib/libflowz_hip.so); "" when the library's path is unknown
static std::string above_library(int up)
{
   Dl_info info;
   std::string p = dladdr((const void*)&above_library, &info) && info.dli_fname ? info.dli_fname : "";
   for (size_t s; up > 0 && !p.empty(); --up) p = (s = p.rfind('/')) == std::string::npos ? std::string(".") : p.substr(0, s);
   return p;
}
std::string library_dir() { return above_library(1); }
// <package>/_kcache (build() pre-fills it); "" when the library's path is unknown
static std::string package_cache_dir() { return above_library(2).empty() ? std::string() : above_library(2) + "/_kcache"; }

// Where code objects are cached: FLOWZ_HIP_CACHE, else the package cache directory when that is writable, else a PER-USER
// directory under /tmp (mode 0700, owner checked: another local user must not be able to plant a code object there).
std::string cache_dir()
{
   if (const char* env = std::getenv("FLOWZ_HIP_CACHE")) return env;
   const std::string pkg = package_cache_dir();
   if (!pkg.empty()) {
      ::mkdir(pkg.c_str(), 0755);
      if (::access(pkg.c_str(), W_OK | X_OK) == 0) return pkg;
   }
   const std::string d = "/tmp/flowz_hip_kcache-" + std::to_string((long)getuid());
   ::mkdir(d.c_str(), 0700);
   struct stat st;
   if (::lstat(d.c_str(), &st) != 0 || !S_ISDIR(st.st_mode) || st.st_uid != getuid() || (st.st_mode & 077) != 0) return "";   // no cache
   return d;
}

// cache file = code object (an ELF: llvm-objdump / readelf still read the file) + trailer {magic, payload bytes, fnv1a of the payload}
struct CacheHeader {
   char magic[8];
   uint64_t size;
   uint64_t hash;
};
static const char kCacheMagic[8] = {'F', 'Z', 'K', 'C', '0', '0', '0', '3'};   // (0002: before the compiler was pinned -- objects of either hiprtc under one name)

static bool cache_load(const std::string& path, std::vector<char>& code, bool may_delete = true)
{
   std::ifstream f(path, std::ios::binary);
   if (!f) return false;
   std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
   CacheHeader h;
   bool ok = raw.size() > sizeof h;
   if (ok) {
      std::memcpy(&h, raw.data() + raw.size() - sizeof h, sizeof h);
      ok = std::memcmp(h.magic, kCacheMagic, 8) == 0 && h.size == raw.size() - sizeof h && h.size > 64 &&
           h.hash == fnv1a_bytes(raw.data(), (size_t)h.size) && std::memcmp(raw.data(), "\x7f" "ELF", 4) == 0;
   }
   if (!ok) {
      if (may_delete) ::unlink(path.c_str());        // truncated / foreign / stale: never try it again
      return false;
   }
   raw.resize((size_t)h.size);
   code.swap(raw);
   return true;
}

static void cache_store(const std::string& dir, const std::string& path, const std::vector<char>& code)
{
   ::mkdir(dir.c_str(), 0755);
   const std::string tmp = path + ".tmp" + std::to_string((long)getpid());
   CacheHeader h;
   std::memcpy(h.magic, kCacheMagic, 8);
   h.size = code.size();
   h.hash = fnv1a_bytes(code.data(), code.size());
   bool ok = false;
   {
      std::ofstream f(tmp, std::ios::binary);
      if (f) {
         f.write(code.data(), (std::streamsize)code.size());
         f.write(reinterpret_cast<const char*>(&h), sizeof h);
         f.close();
         ok = f.good();                              // a short write (ENOSPC ...) must not be installed
      }
   }
   if (!ok || ::rename(tmp.c_str(), path.c_str()) != 0) ::unlink(tmp.c_str());
}

// One field of the kernel's metadata map (code object v3+: an ELF note holding msgpack; one kernel per code object here).
// The key is a msgpack string, the value the msgpack unsigned integer right behind it.
static uint32_t note_uint(const std::vector<char>& code, const char* key)
{
   const size_t kl = std::strlen(key);
   const unsigned char* b = reinterpret_cast<const unsigned char*>(code.data());
   for (size_t i = 1; i + kl + 1 <= code.size(); ++i) {
      if (std::memcmp(b + i, key, kl) != 0) continue;
      const bool fixstr = b[i - 1] == (0xa0u | kl), str8 = i >= 2 && b[i - 2] == 0xd9 && b[i - 1] == kl;
      if (!fixstr && !str8) continue;                         // (the text inside a longer key or a value)
      const unsigned char* v = b + i + kl;
      const size_t left = code.size() - (i + kl);
      if (v[0] <= 0x7f) return v[0];
      if (v[0] == 0xcc && left >= 2) return v[1];
      if (v[0] == 0xcd && left >= 3) return (uint32_t)v[1] << 8 | v[2];
      if (v[0] == 0xce && left >= 5) return (uint32_t)v[1] << 24 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 8 | v[4];
      return 0xFFFFFFFFu;
   }
   return 0;
}

static KernelResources read_resources(const std::vector<char>& code)
{
   KernelResources r;
   r.vgprs = note_uint(code, ".vgpr_count");
   r.agprs = note_uint(code, ".agpr_count");
   r.sgprs = note_uint(code, ".sgpr_count");
   r.scratch_bytes = note_uint(code, ".private_segment_fixed_size");
   r.lds_bytes = note_uint(code, ".group_segment_fixed_size");
   r.vgpr_spills = note_uint(code, ".vgpr_spill_count");
   r.sgpr_spills = note_uint(code, ".sgpr_spill_count");
   return r;
}

// ---- a variant's key, and the one lookup ------------------------------------------------------------------------------
// FNV-1a over (generated source, each build option), finished per compiler (compiler_identity / preferred_identity: who built the
// object).  The 16 hex digits are the kernel's code id and name its code object in the cache.
struct KernelKey {
   uint64_t h;
   KernelKey(const Graph& g, const Variant& v) : h(fnv1a(full_source(g, v))) { for (const char* o : build_options(g, v)) h = fnv1a(o, h); }
   std::string id(const std::string& compiler) const
   {
      char s[17];
      std::snprintf(s, sizeof s, "%016llx", (unsigned long long)fnv1a(compiler, h));
      return s;
   }
};
static std::string cache_file(const std::string& dir, const std::string& code_id) { return dir + "/" + code_id + ".hsaco"; }
static bool cache_in_use(const std::string& dir) { return !std::getenv("FLOWZ_HIP_NO_CACHE") && !dir.empty(); }

// lookups: the installation's compiler first (pre-built objects), then whoever compiles in this process
static std::vector<std::string> compilers_to_look_for()
{
   std::vector<std::string> w{preferred_identity()};
   if (compiler_identity() != w[0]) w.push_back(compiler_identity());
   return w;
}

// Where a variant's object may be, in the order tried: per compiler, the cache directory, then the package cache directory where that
// is another one (a package cache this user cannot write to -- installed by root, pre-filled by build() -- is still read; naming a
// directory with FLOWZ_HIP_CACHE turns that off).  take(path, code id, ours) says whether the file will do; `ours` = of the cache
// directory, where a damaged file may be deleted.  True when one did.
template <class Take>
static bool find_object(const KernelKey& key, Take take)
{
   const std::string dir = cache_dir(), pkg = package_cache_dir();
   if (!cache_in_use(dir)) return false;
   const bool ro_pkg = !pkg.empty() && pkg != dir && !std::getenv("FLOWZ_HIP_CACHE");
   for (const std::string& who : compilers_to_look_for()) {
      const std::string id = key.id(who);
      if (take(cache_file(dir, id), id, true) || (ro_pkg && take(cache_file(pkg, id), id, false))) return true;
   }
   return false;
}

// identity of a variant's CODE (16 hex digits): the name of its code object in the kernel cache under the installation's compiler.  Two
// kernels share it only when generated source, build options and compiler agree -- what counter tables are keyed by (profiles/)
// A kernel this process already holds answers with the id of the object it actually LOADED: a process bound to another hiprtc (a PyTorch
// wheel's) that had to build the kernel itself runs other instructions than the pre-built object of the same variant, and counters
// measured on one must not be attached to the other.
std::string kernel_code_id(fz_program* p, const Variant& v)
{
   {
      std::lock_guard<std::mutex> lock(p->mu);
      auto it = p->kernels.find(v);
      if (it != p->kernels.end() && it->second && it->second->built.load() && !it->second->code_id.empty()) return it->second->code_id;
   }
   return KernelKey(p->g, v).id(preferred_identity());
}

bool kernel_at_hand(fz_program* p, const Variant& v)
{
   {
      std::lock_guard<std::mutex> lock(p->mu);
      auto it = p->kernels.find(v);
      if (it != p->kernels.end() && it->second && it->second->built.load()) return true;
   }
   // (asked before a launch decides what to run: files are neither read nor deleted here)
   return find_object(KernelKey(p->g, v), [](const std::string& path, const std::string&, bool) { return ::access(path.c_str(), R_OK) == 0; });
}

thread_local bool tl_no_jit = false;

// compile, read the resources, name the object after the compiler that built it, store it where the cache is in use
static void build_and_store(fz_program* p, const Variant& v, Kernel& k, const KernelKey& key, bool in_own_process)
{
   k.code = compile_kernel(p->g, v, in_own_process);
   k.res = read_resources(k.code);
   k.code_id = key.id(compiler_identity());
   const std::string dir = cache_dir();
   k.cache_path = cache_in_use(dir) ? cache_file(dir, k.code_id) : std::string();
   if (!k.cache_path.empty()) cache_store(dir, k.cache_path, k.code);
}

// The program mutex is held only to find (or create) the variant's slot; cache lookup, the hiprtc build (seconds) and module
// loading happen under the SLOT's own mutex, so other launches of the program -- other variants, other threads -- go on.
std::shared_ptr<Kernel> get_kernel(fz_program* p, const Variant& v, void** fn_out, bool build_in_own_process)
{
   std::shared_ptr<Kernel> k;
   {
      std::lock_guard<std::mutex> lock(p->mu);
      auto& slot = p->kernels[v];
      if (!slot) slot = std::make_shared<Kernel>();
      k = slot;
   }
   std::lock_guard<std::mutex> build_lock(k->mu);
   if (!k->built.load()) {
      const KernelKey key(p->g, v);
      const bool found = find_object(key, [&](const std::string& path, const std::string& id, bool ours) {
         if (!cache_load(path, k->code, ours)) return false;
         k->code_id = id;
         if (ours) k->cache_path = path;                 // (an object of the package directory: no cache_path, not ours to delete)
         return true;
      });
      if (found) k->res = read_resources(k->code);
      // (the plan measurement a first big launch makes by itself never waits for a build: NoJitScope)
      else if (tl_no_jit) fail(FZ_E_UNSUPPORTED, "kernel not at hand (it would have to be built)");
      else build_and_store(p, v, *k, key, build_in_own_process);
      k->built.store(true);
      manifest_record(p, v);
   }
   if (fn_out) {
      require_device();
      try {
         *fn_out = k->function_on_current_device(kernel_symbol(p->g, v));
      } catch (const Error& er) {
         // a cached code object the DRIVER refuses to load (built for another code-object version, damaged in a way the trailer
         // does not see): delete it, build afresh, store that, try once more.  Anything else -- out of memory, no device, a
         // missing symbol -- is not the file's fault and is passed on.
         const bool image = er.msg.find("hipModuleLoadData") != std::string::npos &&
                            (er.msg.find("invalid") != std::string::npos || er.msg.find("binary") != std::string::npos ||
                             er.msg.find("image") != std::string::npos || er.msg.find("shared object") != std::string::npos);
         if (k->cache_path.empty() || !image) throw;
         ::unlink(k->cache_path.c_str());
         build_and_store(p, v, *k, KernelKey(p->g, v), build_in_own_process);
         *fn_out = k->function_on_current_device(kernel_symbol(p->g, v));
      }
   }
   return k;
}

}  // namespace fz
