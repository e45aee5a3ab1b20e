// Host layer of the kernels compiled at RUN time with hipRTC: what libhj_mi355x.so (hj_rtc.hip: the tiled kernels around a user's Hamiltonian)
// and libhj_hidim.so (hj_hidim.hip: the 5-D / 6-D kernels around one) both need and neither restates -- the loader of libhiprtc.so, the
// compile step, the code-object cache on disk, the module launch and the lock.  Host code only; nothing here knows a kernel's argument block
// or launch shape.  Everything is `static`: each library compiles a copy of its own (own loader handle, own counters, own lock).
//
// The includer defines HJ_RTC_FAIL (its library's  int fail(int code, const char* fmt, ...)) and HIP_TRY before the #include, and may
// define HJ_RTC_WHAT, the noun its messages use for a registration (default "Hamiltonian").
//
// ---- code-object cache on disk: a registered expression is compiled once per (source, kernel headers, options), not once per
// process.  Directory: $HJ_RTC_CACHE ("0" / "off" disables), else $XDG_CACHE_HOME/levelsetpy_amd, else $HOME/.cache/levelsetpy_amd;
// it must belong to the user and not be writable by group or others (a planted file would be code run on the GPU), else the cache
// is off.  File <key>.hjco = "HJCO2\n" + lowered kernel name + "\n" + 16 hex digits: size of the code object + "\n" + 16 hex digits:
// FNV-1a of (key material, code object) + "\n" + code object; key = two FNV-1a hashes (128 bits) of the generated source, the name
// expression, the compile options, the TEXT of every kernel header the source includes, the sizes of the kernel-argument blocks (the
// includer's `abi` words) and the HIP runtime version.  A header that cannot be read turns the cache off (the key would not cover it).
// Written atomically (temporary + rename); a file whose size or checksum does not match is ignored and replaced.
#ifndef HJ_RTC_HOST_H
#define HJ_RTC_HOST_H
#include <dlfcn.h>
#include <errno.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include <hip/hip_runtime.h>

#ifndef HJ_RTC_WHAT
#define HJ_RTC_WHAT "Hamiltonian"
#endif

namespace hj_rtc {

typedef struct _hiprtcProgram* rtcProgram;
struct Rtc {
    void* handle = nullptr;
    int (*CreateProgram)(rtcProgram*, const char*, const char*, int, const char**, const char**) = nullptr;
    int (*CompileProgram)(rtcProgram, int, const char**) = nullptr;
    int (*AddNameExpression)(rtcProgram, const char*) = nullptr;
    int (*GetLoweredName)(rtcProgram, const char*, const char**) = nullptr;
    int (*GetCodeSize)(rtcProgram, size_t*) = nullptr;
    int (*GetCode)(rtcProgram, char*) = nullptr;
    int (*GetProgramLogSize)(rtcProgram, size_t*) = nullptr;
    int (*GetProgramLog)(rtcProgram, char*) = nullptr;
    int (*DestroyProgram)(rtcProgram*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
static Rtc g_rtc;

static int rtc_load(const char* path) {
    if (g_rtc.handle) return HJ_OK;
    const char* names[] = {path, "libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"};
    void* h = nullptr;
    for (const char* n : names) {
        if (!n || !*n) continue;
        h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (h) break;
    }
    if (!h) return HJ_RTC_FAIL(HJ_ESTATE, "cannot dlopen hipRTC: %s", dlerror());
#define HJ_SYM(field, name)                                                     \
    *(void**)(&g_rtc.field) = dlsym(h, name);                                   \
    if (!g_rtc.field) return HJ_RTC_FAIL(HJ_ESTATE, "hipRTC symbol %s missing", name);
    HJ_SYM(CreateProgram, "hiprtcCreateProgram")
    HJ_SYM(CompileProgram, "hiprtcCompileProgram")
    HJ_SYM(AddNameExpression, "hiprtcAddNameExpression")
    HJ_SYM(GetLoweredName, "hiprtcGetLoweredName")
    HJ_SYM(GetCodeSize, "hiprtcGetCodeSize")
    HJ_SYM(GetCode, "hiprtcGetCode")
    HJ_SYM(GetProgramLogSize, "hiprtcGetProgramLogSize")
    HJ_SYM(GetProgramLog, "hiprtcGetProgramLog")
    HJ_SYM(DestroyProgram, "hiprtcDestroyProgram")
    HJ_SYM(GetErrorString, "hiprtcGetErrorString")
#undef HJ_SYM
    g_rtc.handle = h;
    return HJ_OK;
}

// Every entry point that looks at or extends a library's tables of registered Hamiltonians and their kernels takes this lock: kernels are
// compiled lazily at the first launch, and several host threads (virtual ranks in one process: tests/fuzz_slabs.py found the race in round 5
// -- eight threads met in the first compile of the same kernel) must see either no kernel or a complete one.  The launches themselves are
// asynchronous: the lock is held for microseconds once the kernels exist.
static std::recursive_mutex g_rtc_mu;
#define HJ_RTC_LOCK std::lock_guard<std::recursive_mutex> hj_rtc_guard(::hj_rtc::g_rtc_mu)

static unsigned long long fnv1a(const void* data, size_t n, unsigned long long h = 1469598103934665603ull) {
    const unsigned char* p = (const unsigned char*)data;
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}
static bool read_file(const std::string& path, std::string& out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    char buf[65536];
    size_t n;
    out.clear();
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out.append(buf, n);
    fclose(f);
    return true;
}
static std::string cache_dir() {
    const char* e = getenv("HJ_RTC_CACHE");
    if (e && (!strcmp(e, "0") || !strcmp(e, "off"))) return "";
    std::string d;
    if (e && *e) d = e;
    else if ((e = getenv("XDG_CACHE_HOME")) && *e) d = std::string(e) + "/levelsetpy_amd";
    else if ((e = getenv("HOME")) && *e) d = std::string(e) + "/.cache/levelsetpy_amd";
    else return "";
    // mkdir -p of the last two components (the parents of a cache home exist)
    const size_t cut = d.find_last_of('/');
    if (cut != std::string::npos && cut > 0) (void)mkdir(d.substr(0, cut).c_str(), 0700);
    if (mkdir(d.c_str(), 0700) != 0 && errno != EEXIST) return "";
    struct stat st;
    if (stat(d.c_str(), &st) != 0 || !S_ISDIR(st.st_mode) || st.st_uid != geteuid() || (st.st_mode & (S_IWGRP | S_IWOTH))) return "";
    return d;
}

// What one library's generated sources have in common: the headers they can include (paths relative to the include directory, each
// beginning with '/') and the sizes of the kernel-argument blocks.
struct Unit {
    std::vector<const char*> headers;
    std::vector<unsigned long long> abi;
};

// hash of the text of every header the generated source can include; ok = false if one of them cannot be read
static unsigned long long headers_hash(const Unit& unit, const std::string& include_dir, unsigned long long seed, bool& ok) {
    static std::map<std::string, std::pair<unsigned long long, bool>> memo;
    const std::string key = include_dir + "#" + std::to_string(seed);
    auto it = memo.find(key);
    if (it != memo.end()) { ok = it->second.second; return it->second.first; }
    unsigned long long h = seed;
    ok = true;
    std::string text;
    for (const char* f : unit.headers) {
        if (read_file(include_dir + f, text)) h = fnv1a(text.data(), text.size(), h);
        else {
            // the key cannot cover this header's text: the caller keeps the disk cache OFF for this include directory (and says so once)
            ok = false;
            fprintf(stderr, "[hj] run-time kernels: cannot read %s%s -- the on-disk code-object cache is disabled\n", include_dir.c_str(), f);
        }
    }
    memo[key] = std::make_pair(h, ok);
    return h;
}
static int g_rtc_cache_hits = 0, g_rtc_compiles = 0;

static const char* const BASE_OPTS[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "-DHJ_RTC=1"};

// the compiler's message of a failed compile, cut to what an error record holds
static std::string program_log(rtcProgram prog) {
    size_t n = 0;
    std::string log;
    if (g_rtc.GetProgramLogSize(prog, &n) == 0 && n > 1) { log.resize(n); (void)g_rtc.GetProgramLog(prog, &log[0]); }
    if (log.size() > 3000) log = log.substr(0, 3000) + " ...";
    return log;
}

// One kernel (the instantiation `name_expr` names) of the translation unit `src`, loaded on the CURRENT device: from the disk cache, else
// compiled now and written there.  `what`: the registration's name, for the message.
static int rtc_build(const Unit& unit, const std::string& src, const std::string& name_expr, const std::string& what, const std::string& include_dir,
                     const std::string& rtc_path, hipModule_t& mod, hipFunction_t& fn) {
    std::string cache_file;
    unsigned long long key_lo = 0;
    {
        const std::string dir = cache_dir();
        if (!dir.empty()) {
            unsigned long long h[2];
            bool ok = true;
            for (int w = 0; w < 2; ++w) {
                const unsigned long long seed = w == 0 ? 1469598103934665603ull : 0x9e3779b97f4a7c15ull;
                unsigned long long x = fnv1a(src.data(), src.size(), seed);
                x = fnv1a(name_expr.data(), name_expr.size(), x);
                for (const char* o : BASE_OPTS) x = fnv1a(o, strlen(o), x);
                bool okh = true;
                const unsigned long long hh = headers_hash(unit, include_dir, seed, okh);
                ok = ok && okh;
                x = fnv1a(&hh, sizeof(hh), x);
                x = fnv1a(unit.abi.data(), sizeof(unsigned long long) * unit.abi.size(), x);
                int rtv = 0;                                   // a new ROCm release compiles again
                (void)hipRuntimeGetVersion(&rtv);
                x = fnv1a(&rtv, sizeof(rtv), x);
                h[w] = x;
            }
            if (ok) {
                key_lo = h[0];
                char nm[64];
                snprintf(nm, sizeof(nm), "/%016llx%016llx.hjco", h[0], h[1]);
                cache_file = dir + nm;
                std::string blob;
                if (read_file(cache_file, blob) && blob.compare(0, 6, "HJCO2\n") == 0) {
                    const size_t n1 = blob.find('\n', 6);
                    if (n1 != std::string::npos && blob.size() >= n1 + 1 + 17 + 17) {
                        const std::string kname = blob.substr(6, n1 - 6);
                        const unsigned long long want_size = strtoull(blob.substr(n1 + 1, 16).c_str(), nullptr, 16);
                        const unsigned long long want_sum = strtoull(blob.substr(n1 + 18, 16).c_str(), nullptr, 16);
                        const size_t off = n1 + 1 + 17 + 17;
                        if (blob[n1 + 17] == '\n' && blob[n1 + 34] == '\n' && blob.size() - off == want_size &&
                            fnv1a(blob.data() + off, blob.size() - off, key_lo) == want_sum &&
                            hipModuleLoadData(&mod, blob.data() + off) == hipSuccess &&
                            hipModuleGetFunction(&fn, mod, kname.c_str()) == hipSuccess) {
                            ++g_rtc_cache_hits;
                            return HJ_OK;
                        }
                        (void)hipGetLastError();
                        mod = nullptr; fn = nullptr;
                    }
                }
            }
        }
    }
    int rc = rtc_load(rtc_path.empty() ? nullptr : rtc_path.c_str());
    if (rc) return rc;
    ++g_rtc_compiles;
    rtcProgram prog = nullptr;
    int e = g_rtc.CreateProgram(&prog, src.c_str(), "hj_user_ham.hip", 0, nullptr, nullptr);
    if (e) return HJ_RTC_FAIL(HJ_EHIP, "hiprtcCreateProgram: %s", g_rtc.GetErrorString(e));
    e = g_rtc.AddNameExpression(prog, name_expr.c_str());
    const std::string inc1 = "-I" + include_dir, inc2 = "-I" + include_dir + "/../../include";
    const char* opts[] = {BASE_OPTS[0], BASE_OPTS[1], BASE_OPTS[2], BASE_OPTS[3], inc1.c_str(), inc2.c_str(), BASE_OPTS[4]};
    if (!e) e = g_rtc.CompileProgram(prog, (int)(sizeof(opts) / sizeof(opts[0])), opts);
    if (e) {
        const std::string log = program_log(prog);
        (void)g_rtc.DestroyProgram(&prog);
        return HJ_RTC_FAIL(HJ_EINVAL, "the " HJ_RTC_WHAT " '%s' does not compile (%s):\n%s", what.c_str(), g_rtc.GetErrorString(e), log.c_str());
    }
    const char* lowered = nullptr;
    e = g_rtc.GetLoweredName(prog, name_expr.c_str(), &lowered);
    size_t n = 0;
    if (!e) e = g_rtc.GetCodeSize(prog, &n);
    std::vector<char> code(n);
    if (!e) e = g_rtc.GetCode(prog, code.data());
    const std::string kname = lowered ? lowered : "";
    (void)g_rtc.DestroyProgram(&prog);
    if (e) return HJ_RTC_FAIL(HJ_EHIP, "hipRTC: %s", g_rtc.GetErrorString(e));
    HIP_TRY(hipModuleLoadData(&mod, code.data()));
    HIP_TRY(hipModuleGetFunction(&fn, mod, kname.c_str()));
    if (!cache_file.empty()) {
        char tmpn[64];
        snprintf(tmpn, sizeof(tmpn), ".tmp%ld", (long)getpid());
        const std::string tmp = cache_file + tmpn;
        FILE* f = fopen(tmp.c_str(), "wb");
        if (f) {
            char meta[64];
            snprintf(meta, sizeof(meta), "%016llx\n%016llx\n", (unsigned long long)code.size(), fnv1a(code.data(), code.size(), key_lo));
            bool ok = fwrite("HJCO2\n", 1, 6, f) == 6 && fwrite(kname.data(), 1, kname.size(), f) == kname.size() && fputc('\n', f) != EOF &&
                      fwrite(meta, 1, 34, f) == 34 && fwrite(code.data(), 1, code.size(), f) == code.size();
            ok = (fclose(f) == 0) && ok;
            if (!ok || rename(tmp.c_str(), cache_file.c_str()) != 0) (void)remove(tmp.c_str());
        }
    }
    return HJ_OK;
}

// compile the instantiations `names` of `src` without loading or launching anything (needs no GPU: hipRTC cross-compiles for gfx950)
static int rtc_compile_check(const std::string& src, const std::vector<std::string>& names, const std::string& what, const std::string& include_dir,
                             const std::string& rtc_path) {
    int rc = rtc_load(rtc_path.empty() ? nullptr : rtc_path.c_str());
    if (rc) return rc;
    if (const char* dump = getenv("HJ_RTC_DUMP")) {        // the translation unit hipRTC is given, for a look at it (or an offline hipcc -S)
        if (FILE* f = fopen(dump, "w")) { fputs(src.c_str(), f); fclose(f); }
    }
    rtcProgram prog = nullptr;
    int e = g_rtc.CreateProgram(&prog, src.c_str(), "hj_user_ham.hip", 0, nullptr, nullptr);
    if (e) return HJ_RTC_FAIL(HJ_EHIP, "hiprtcCreateProgram: %s", g_rtc.GetErrorString(e));
    for (const std::string& n : names)
        if (!e) e = g_rtc.AddNameExpression(prog, n.c_str());
    const std::string inc1 = "-I" + include_dir, inc2 = "-I" + include_dir + "/../../include";
    const char* opts[] = {BASE_OPTS[0], BASE_OPTS[1], BASE_OPTS[2], BASE_OPTS[3], inc1.c_str(), inc2.c_str(), BASE_OPTS[4]};
    if (!e) e = g_rtc.CompileProgram(prog, (int)(sizeof(opts) / sizeof(opts[0])), opts);
    std::string log;
    if (e) log = program_log(prog);
    (void)g_rtc.DestroyProgram(&prog);
    if (e) return HJ_RTC_FAIL(HJ_EINVAL, "the " HJ_RTC_WHAT " '%s' does not compile (%s):\n%s", what.c_str(), g_rtc.GetErrorString(e), log.c_str());
    return HJ_OK;
}

static int module_launch(hipFunction_t fn, unsigned grid, unsigned block, size_t lds, hipStream_t st, void* args, size_t nbytes) {
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &nbytes, HIP_LAUNCH_PARAM_END};
    HIP_TRY(hipModuleLaunchKernel(fn, grid, 1, 1, block, 1, 1, (unsigned)lds, st, nullptr, cfg));
    return HJ_OK;
}

}  // namespace hj_rtc
#endif
