// jit_cache.h — from a generated source (jit.h) to a loaded kernel: hiprtc compilation for gfx950 and the code objects kept on disk.
#pragma once
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>

namespace paml_amd {

struct JitKernel {
   hipModule_t mod = nullptr;
   hipFunction_t fn = nullptr;
   std::string key;
   size_t n_ops = 0;
};

inline std::string jit_source_dir()
{
   if (const char *e = getenv("PAML_AMD_CSRC")) return e;      // (a variant library built somewhere else: tools/build_variant.sh, PAML_AMD_LIB)
   Dl_info info;
   if (dladdr((const void *)&jit_source_dir, &info) && info.dli_fname) {
      std::string so = info.dli_fname;                 // .../paml_amd/lib/libpaml_amd.so
      const size_t cut = so.rfind('/');
      const std::string libdir = cut == std::string::npos ? "." : so.substr(0, cut);
      return libdir + "/../csrc";
   }
   return "paml_amd/csrc";
}

// Compile `src` for gfx950 (works without a GPU).  Returns 0 on success; `log` gets the compiler output.
// Code objects are kept on disk, keyed by a hash of the generated source, of the header it includes, of the optimisation
// level and of the hiprtc version: a tree seen before (another run of the same analysis) costs a file read instead of
// seconds of hiprtc (0.2 - 19 s per topology, profiles/r01_big_trees.jsonl).  Two places are looked at:
//   <library dir>/jit/         read-only: code objects built together with the library (__graft_entry__.build() fills it for
//                              the benchmark's trees), so a fresh machine does not start with a compile;
//   the user's cache           read-write: $PAML_AMD_JIT_CACHE, else $XDG_CACHE_HOME/paml_amd/jit, else $HOME/.cache/paml_amd/jit;
//                              PAML_AMD_JIT_CACHE=0 (or empty) switches it off.
inline const char *jit_opt_level() { return "-O3"; }

inline std::string jit_cache_name(const std::string &src)
{
   unsigned long long h = 1469598103934665603ull;
   auto mix = [&](const std::string &t) { for (unsigned char ch : t) { h ^= ch; h *= 1099511628211ull; } };
   mix(src);
   {  // the header the source includes is part of the program
      FILE *f = fopen((jit_source_dir() + "/device_common.h").c_str(), "rb");
      if (f) { char buf[4096]; size_t n; while ((n = fread(buf, 1, sizeof(buf), f)) > 0) mix(std::string(buf, n)); fclose(f); }
   }
   mix(jit_opt_level());
   int major = 0, minor = 0;
   (void)hiprtcVersion(&major, &minor);
   mix("hiprtc" + std::to_string(major) + "." + std::to_string(minor));
   char name[64];
   snprintf(name, sizeof(name), "%016llx.gfx950.hsaco", h);
   return name;
}

inline bool jit_mkdirs(const std::string &dir)      // mkdir -p without a shell
{
   for (size_t i = 1; i <= dir.size(); i++)
      if (i == dir.size() || dir[i] == '/') {
         const std::string sub = dir.substr(0, i);
         if (mkdir(sub.c_str(), 0777) != 0 && errno != EEXIST) return false;
      }
   return true;
}

inline std::string jit_shipped_dir() { return jit_source_dir() + "/../lib/jit"; }

inline std::string jit_user_cache_dir()
{
   const char *c = getenv("PAML_AMD_JIT_CACHE");
   if (c) return (!*c || !strcmp(c, "0")) ? std::string() : std::string(c);
   if (const char *x = getenv("XDG_CACHE_HOME"))
      if (*x) return std::string(x) + "/paml_amd/jit";
   if (const char *hm = getenv("HOME"))
      if (*hm) return std::string(hm) + "/.cache/paml_amd/jit";
   return std::string();
}

inline bool jit_read_file(const std::string &path, std::vector<char> *code)
{
   FILE *f = fopen(path.c_str(), "rb");
   if (!f) return false;
   fseek(f, 0, SEEK_END);
   const long n = ftell(f);
   rewind(f);
   code->resize(n > 0 ? n : 0);
   const bool ok = n > 0 && fread(code->data(), 1, n, f) == (size_t)n;
   fclose(f);
   return ok;
}

inline void jit_write_file(const std::string &dir, const std::string &name, const std::vector<char> &code)
{
   if (dir.empty() || !jit_mkdirs(dir)) return;
   const std::string path = dir + "/" + name, tmp = path + ".tmp" + std::to_string((long)getpid());      // write beside, then rename:
   FILE *f = fopen(tmp.c_str(), "wb");                                                                    // readers never see a partial file
   if (!f) return;
   const bool ok = fwrite(code.data(), 1, code.size(), f) == code.size();
   fclose(f);
   if (!ok || rename(tmp.c_str(), path.c_str()) != 0) remove(tmp.c_str());
}

inline int jit_compile_code(const std::string &src, std::vector<char> *code, std::string *log, const char *store_dir = nullptr)
{
   const std::string name = jit_cache_name(src), user = jit_user_cache_dir();
   if (const char *d = getenv("PAML_AMD_JIT_SRC_DIR")) {      // debugging: every source that reaches the compiler (or its cache), by cache name
      if (FILE *f = fopen((std::string(d) + "/" + name + ".hip").c_str(), "wb")) { fwrite(src.data(), 1, src.size(), f); fclose(f); }
   }
   if (!store_dir) {
      if (jit_read_file(jit_shipped_dir() + "/" + name, code)) return 0;
      if (!user.empty() && jit_read_file(user + "/" + name, code)) return 0;
   }
   hiprtcProgram prog;
   if (hiprtcCreateProgram(&prog, src.c_str(), "prune_jit.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) {
      *log = "hiprtcCreateProgram failed";
      return -1;
   }
   const std::string inc = "-I" + jit_source_dir();
   std::vector<const char *> opts = {"--offload-arch=gfx950", jit_opt_level(), "-std=c++17", inc.c_str()};
   const hiprtcResult r = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
   size_t ls = 0;
   hiprtcGetProgramLogSize(prog, &ls);
   if (ls > 1) {
      log->resize(ls);
      hiprtcGetProgramLog(prog, &(*log)[0]);
   }
   if (r != HIPRTC_SUCCESS) {
      hiprtcDestroyProgram(&prog);
      return -1;
   }
   size_t cs = 0;
   hiprtcGetCodeSize(prog, &cs);
   code->resize(cs);
   hiprtcGetCode(prog, code->data());
   hiprtcDestroyProgram(&prog);
   jit_write_file(store_dir ? std::string(store_dir) : user, name, *code);
   return 0;
}

// The code object of `src` if it is already on disk (the library's lib/jit or the user's cache): no compilation.
inline bool jit_cached_code(const std::string &src, std::vector<char> *code)
{
   const std::string name = jit_cache_name(src), user = jit_user_cache_dir();
   if (jit_read_file(jit_shipped_dir() + "/" + name, code)) return true;
   return !user.empty() && jit_read_file(user + "/" + name, code);
}

inline int jit_load_code(const std::vector<char> &code, JitKernel *out)
{
   if (hipModuleLoadData(&out->mod, code.data()) != hipSuccess) return -1;
   if (hipModuleGetFunction(&out->fn, out->mod, "prune_jit") != hipSuccess) return -1;
   return 0;
}

}  // namespace paml_amd
