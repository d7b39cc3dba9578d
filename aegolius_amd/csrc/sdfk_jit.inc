// JIT plumbing: the on-disk cache of code objects, hiprtc options and keys, the compiler child process, the build
// worker, code objects (per process) and modules (per device), and the residency of a program on a device.
// Included by sdfk.hip.
// On-disk cache of hiprtc code objects, ON by default: a new process loads the kernels of tree / chain shapes it has
// seen before instead of compiling them. Directory: $SDFK_CACHE_DIR, else $XDG_CACHE_HOME/sdfk, else $HOME/.cache/sdfk;
// SDFK_CACHE_DIR= (empty), "off" or "0" disables it. The file name is a 64-bit FNV-1a hash of the source, the options
// and the hiprtc version, plus the source length. A cache that cannot be created, read or written is never an error.
static std::string rtc_cache_dir() {
    static const std::string dir = [] {
        std::string d;
        if (const char* e = getenv("SDFK_CACHE_DIR")) {
            d = e;
            if (d.empty() || d == "off" || d == "0") return std::string();
        } else if (const char* x = getenv("XDG_CACHE_HOME"); x && *x) {
            d = std::string(x) + "/sdfk";
        } else if (const char* h = getenv("HOME"); h && *h) {
            (void)mkdir((std::string(h) + "/.cache").c_str(), 0700);
            d = std::string(h) + "/.cache/sdfk";
        } else {
            return std::string();
        }
        (void)mkdir(d.c_str(), 0700);
        return d;
    }();
    return dir;
}
static std::string rtc_cache_path(const std::string& src, const std::string& opts) {
    const std::string dir = rtc_cache_dir();
    if (dir.empty()) return std::string();
    int major = 0, minor = 0;
    (void)hiprtcVersion(&major, &minor);
    unsigned long long h = 1469598103934665603ull;
    auto mix = [&](const std::string& t) {
        for (unsigned char c : t) {
            h ^= c;
            h *= 1099511628211ull;
        }
    };
    mix(src);
    mix(opts);
    mix(std::to_string(major) + "." + std::to_string(minor) + "/abi" + std::to_string(SDFK_ABI_VERSION));
    char name[96];
    snprintf(name, sizeof name, "/sdfk-%016llx-%zu.co", h, src.size());
    return dir + name;
}
// File = code object + 24-byte trailer {magic, payload length, FNV-1a of the payload}: a truncated or foreign file is
// never handed to hipModuleLoadData (it is deleted instead).
static const unsigned long long kCacheMagic = 0x53444643'4f424a31ull;           // "SDFCOBJ1"
static unsigned long long fnv1a(const char* p, size_t n) {
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) {
        h ^= (unsigned char)p[i];
        h *= 1099511628211ull;
    }
    return h;
}
static bool rtc_cache_read(const std::string& path, std::vector<char>* out) {
    if (path.empty()) return false;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    bool ok = false;
    if (fseek(f, 0, SEEK_END) == 0) {
        const long size = ftell(f);
        if (size > 24 && fseek(f, 0, SEEK_SET) == 0) {
            out->resize((size_t)size);
            ok = fread(out->data(), 1, (size_t)size, f) == (size_t)size;
            if (ok) {
                unsigned long long tr[3];
                memcpy(tr, out->data() + size - 24, 24);
                ok = tr[0] == kCacheMagic && tr[1] == (unsigned long long)(size - 24) && tr[2] == fnv1a(out->data(), (size_t)size - 24);
                out->resize((size_t)size - 24);
            }
        }
    }
    fclose(f);
    if (!ok) {
        out->clear();
        (void)remove(path.c_str());                            // truncated / corrupt / older format: rebuilt and rewritten
    } else {
        (void)utimes(path.c_str(), nullptr);                   // most recently used (the eviction below goes by mtime)
    }
    return ok;
}
// keep the directory below SDFK_CACHE_MAX_MB (default 512): oldest files go first, down to three quarters of the cap
static void rtc_cache_evict(const std::string& dir) {
    static const long long cap = [] {
        const char* e = getenv("SDFK_CACHE_MAX_MB");
        const long long v = e ? atoll(e) : 512;
        return (v > 0 ? v : 512) * (1ll << 20);
    }();
    DIR* d = opendir(dir.c_str());
    if (!d) return;
    std::vector<std::pair<long long, std::pair<std::string, long long>>> files;   // (mtime, (path, size))
    long long total = 0;
    while (dirent* e = readdir(d)) {
        const std::string name = e->d_name;
        if (name.compare(0, 5, "sdfk-") != 0 || name.compare(0, 9, "sdfk-rtc-") == 0) continue;   // (not the hand-over directories of builds in flight)
        struct stat st;
        const std::string path = dir + "/" + name;
        if (stat(path.c_str(), &st) != 0) continue;
        total += (long long)st.st_size;
        files.push_back({(long long)st.st_mtime, {path, (long long)st.st_size}});
    }
    closedir(d);
    if (total <= cap) return;
    std::sort(files.begin(), files.end());
    for (const auto& f : files) {
        if (total <= cap / 4 * 3) break;
        if (remove(f.second.first.c_str()) == 0) total -= f.second.second;
    }
}
static void rtc_cache_write(const std::string& path, const std::vector<char>& co) {
    if (path.empty() || co.empty()) return;
    const std::string tmp = path + ".tmp" + std::to_string((long long)getpid());
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) return;                                            // a cache that cannot be written is no error
    const unsigned long long tr[3] = {kCacheMagic, (unsigned long long)co.size(), fnv1a(co.data(), co.size())};
    bool ok = fwrite(co.data(), 1, co.size(), f) == co.size() && fwrite(tr, 1, sizeof tr, f) == sizeof tr;
    ok = (fclose(f) == 0) && ok;                               // (a short write on a full disk may only show here)
    if (!ok || rename(tmp.c_str(), path.c_str()) != 0) (void)remove(tmp.c_str());   // atomic: readers never see a partial file
    else rtc_cache_evict(rtc_cache_dir());
}

static std::mutex g_rtc_mu;   // hiprtc and hipModuleLoadData: one thread at a time (see BuildWorker)
// (experiments: "-DSDFK_TWAVES=n" / "-DSDFK_RWBRICKS=n" inside the extra build switches override the launch geometry)
static std::atomic<int> g_twaves_override{0}, g_rwbricks_override{0};
static std::atomic<int> g_rwaves_override{0};
// extra -D switches for the generated source (experiments): SDFK_RTC_DEFS="-DSDFK_TWAVES=2 ..." or sdfk_debug_set_rtc_defs
static std::mutex g_defs_mu;
static std::string g_rtc_defs = [] { const char* e = getenv("SDFK_RTC_DEFS"); return std::string(e ? e : ""); }();
extern "C" void sdfk_debug_set_rtc_defs(const char* defs) {
    std::lock_guard<std::mutex> lk(g_defs_mu);
    std::string rest;
    int tw = 0, rwb = 0, rwv = 0;
    const std::string all = defs ? defs : "";
    size_t pos = 0;
    while (pos < all.size()) {
        size_t sp = all.find(' ', pos);
        if (sp == std::string::npos) sp = all.size();
        const std::string tok = all.substr(pos, sp - pos);
        if (tok.compare(0, 14, "-DSDFK_TWAVES=") == 0) tw = atoi(tok.c_str() + 14);
        else if (tok.compare(0, 16, "-DSDFK_RWBRICKS=") == 0) rwb = atoi(tok.c_str() + 16);
        else if (tok.compare(0, 14, "-DSDFK_RWAVES=") == 0) rwv = atoi(tok.c_str() + 14);
        else if (!tok.empty()) rest += tok + " ";
        pos = sp + 1;
    }
    g_twaves_override = (tw >= 1 && tw <= 16) ? tw : 0;
    g_rwbricks_override = (rwb >= 1 && rwb <= 15) ? rwb : 0;
    g_rwaves_override = (rwv >= 1 && rwv <= 16) ? rwv : 0;
    g_rtc_defs = rest;
}
// geo: bricks per wave | waves per workgroup << 4 of the row-block kernel (rows_geo)
static std::vector<std::string> rtc_options(int geo) {
    const int rwb = geo & 15, rwaves = ((geo >> 4) & 0xff) ? ((geo >> 4) & 0xff) : 4;
    const bool big = (geo >> 16) & 1;
    const char* opt = getenv("SDFK_RTC_OPT");                 // experiments: "-O1" ... (the cache key carries the options)
    std::vector<std::string> o = {"--offload-arch=gfx950", (opt && opt[0] == '-') ? opt : "-O3", "-ffp-contract=off", "-std=c++17",
                                  // -fno-honor-nans: v_min/v_max without the canonicalising pre-op. -mno-amdgpu-ieee (same
                                  // flags as the hipcc build of the interpreter kernel: both flavours stay bit-identical)
                                  // keeps the device library's sincos / atan2 / pow out of line — the inliner refuses
                                  // across the attribute — which is what a 50-primitive 2-D tree wants: 296 KB of code
                                  // instead of 490 KB, 10 s of compile instead of 15 s, 1.19 vs 1.22 ms at 16385^2
                                  "-fno-honor-nans", "-mno-amdgpu-ieee",
                                  "-DSDFK_TWAVES=" + std::to_string(tile_waves()), "-DSDFK_WBRICKS=" + std::to_string(tile_wbricks()),
                                  "-DSDFK_RWBRICKS=" + std::to_string(rwb), "-DSDFK_RWAVES=" + std::to_string(rwaves)};
    if (big) {
        // Big programs (round 4): hiprtc's time grows with the square of a straight-line program, and -ftime-report on a
        // 599-instruction tree names the pass: CodeGenPrepare, 458 of 630 s (then VectorCombine, 31 of the remaining 151).
        // Without the two a row-block build takes 30 s instead of 250 at 599 instructions, line bricks 33 s at 1199
        // instead of 105 (profiles/r04_build_time.txt). CodeGenPrepare is worth 2 % on the north-star tree and 12 % on the
        // 20-primitive one (profiles/r04_nocgp.txt) — so small programs keep it — but a culled kernel without it is still
        // several times the interpreter kernel, which is what served these programs before. Same FP semantics: same bits.
        o.push_back("-mllvm");
        o.push_back("-disable-cgp");
        o.push_back("-mllvm");
        o.push_back("-disable-vector-combine");
    }
    if (const char* extra = getenv("SDFK_RTC_EXTRA")) {       // experiments: raw compiler options, space-separated
        std::string e = extra;
        size_t q = 0;
        while (q < e.size()) {
            size_t sp = e.find(' ', q);
            if (sp == std::string::npos) sp = e.size();
            if (sp > q) o.push_back(e.substr(q, sp - q));
            q = sp + 1;
        }
    }
    std::string all;
    {
        std::lock_guard<std::mutex> lk(g_defs_mu);
        all = g_rtc_defs;
    }
    size_t pos = 0;
    while (pos < all.size()) {
        size_t sp = all.find(' ', pos);
        if (sp == std::string::npos) sp = all.size();
        if (sp > pos && all.compare(pos, 2, "-D") == 0) o.push_back(all.substr(pos, sp - pos));
        pos = sp + 1;
    }
    return o;
}
static std::string rtc_option_key(int rwb) {
    std::string k;
    for (const std::string& o : rtc_options(rwb)) k += o + " ";
    return k;
}
static int rtc_compile_uncached(const std::string& src, std::vector<char>* out, std::string* log, int rwb) {
    hiprtcProgram prog = nullptr;
    if (hiprtcCreateProgram(&prog, src.c_str(), "sdfk_spec.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) {
        *log = "hiprtcCreateProgram failed";
        return -1;
    }
    const std::vector<std::string> o = rtc_options(rwb);
    std::vector<const char*> opts;
    for (const std::string& x : o) opts.push_back(x.c_str());
    hiprtcResult r = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
    size_t ls = 0;
    hiprtcGetProgramLogSize(prog, &ls);
    if (ls > 1) {
        log->resize(ls);
        hiprtcGetProgramLog(prog, &(*log)[0]);
    }
    if (r != HIPRTC_SUCCESS) {
        *log = std::string("hiprtc: ") + hiprtcGetErrorString(r) + "\n" + *log;
        hiprtcDestroyProgram(&prog);
        return -1;
    }
    size_t cs = 0;
    hiprtcGetCodeSize(prog, &cs);
    out->resize(cs);
    hiprtcGetCode(prog, out->data());
    hiprtcDestroyProgram(&prog);
    return 0;
}
// ---- hiprtc in a child process (background builds) -------------------------------------------------------------------
// hiprtcCompileProgram holds comgr's process-wide mutex for the whole build; a dlopen of any library with HIP fat
// binaries on another thread of the same process (`import torch`) deadlocks against it — loader lock -> comgr mutex there,
// comgr mutex -> loader lock here (profiles/r03_hang_import_during_build.txt). Builds that run BESIDE the caller
// therefore run in aegolius_amd/sdfk_rtc_helper (csrc/sdfk_rtc_helper.c): no GPU, no shared lock. Builds the caller
// waits for stay in-process (the caller cannot dlopen while it waits). No helper next to the library: no background
// builds — the call waits.
extern char** environ;
static std::string rtc_helper_path() {
    static const std::string path = [] {
        if (const char* e = getenv("SDFK_RTC_HELPER")) return std::string(strcmp(e, "off") && strcmp(e, "0") ? e : "");
        Dl_info info;
        if (!dladdr((void*)&sdfk_abi_version, &info) || !info.dli_fname) return std::string();
        std::string p = info.dli_fname;
        const size_t slash = p.rfind('/');
        p = (slash == std::string::npos ? std::string(".") : p.substr(0, slash)) + "/sdfk_rtc_helper";
        return access(p.c_str(), X_OK) == 0 ? p : std::string();
    }();
    return path;
}
static std::string rtc_library_path() {                        // the hiprtc THIS process uses (torch's or the system's)
    Dl_info info;
    if (!dladdr((void*)&hiprtcCompileProgram, &info) || !info.dli_fname) return std::string();
    return info.dli_fname;
}
static bool rtc_helper_available() { return !rtc_helper_path().empty() && !rtc_library_path().empty(); }
static std::atomic<bool> g_cancel_builds{false};              // set by sdfk_jit_cancel: running compiler children are killed, queued builds dropped
static int rtc_compile_external(const std::string& src, std::vector<char>* out, std::string* log, int rwb) {
    static std::atomic<unsigned> serial{0};
    const std::string helper = rtc_helper_path(), lib = rtc_library_path();
    if (helper.empty() || lib.empty()) {
        *log = "sdfk_rtc_helper is not available";
        return -2;
    }
    std::string dir = rtc_cache_dir();
    if (dir.empty()) {
        const char* t = getenv("TMPDIR");
        dir = (t && *t) ? t : "/tmp";
    }
    // the hand-over files live in a directory of their own that mkdtemp creates (mode 0700, unpredictable name): nobody
    // can plant a file or a link where the source is written or the code object is read, two processes with the same pid in
    // different namespaces that share the cache directory cannot meet, and the cache eviction skips the "sdfk-rtc-" prefix
    (void)serial;
    std::string priv = dir + "/sdfk-rtc-XXXXXX";
    if (!mkdtemp(&priv[0])) {
        *log = "cannot create a private directory under " + dir + ": " + strerror(errno);
        return -2;
    }
    const std::string srcf = priv + "/src.hip", outf = priv + "/out.co";
    auto cleanup = [&] {
        (void)remove(srcf.c_str());
        (void)remove(outf.c_str());
        (void)remove((outf + ".tmp").c_str());
        (void)remove((outf + ".log").c_str());
        (void)rmdir(priv.c_str());
    };
    {
        const int fd = open(srcf.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_CLOEXEC, 0600);
        FILE* f = fd >= 0 ? fdopen(fd, "wb") : nullptr;
        if (!f && fd >= 0) close(fd);
        const bool ok = f && fwrite(src.data(), 1, src.size(), f) == src.size();
        if (!f || fclose(f) != 0 || !ok) {
            cleanup();
            *log = "cannot write " + srcf;
            return -2;
        }
    }
    const std::vector<std::string> o = rtc_options(rwb);
    std::vector<char*> argv = {const_cast<char*>(helper.c_str()), const_cast<char*>(lib.c_str()), const_cast<char*>(srcf.c_str()),
                               const_cast<char*>(outf.c_str())};
    for (const std::string& x : o) argv.push_back(const_cast<char*>(x.c_str()));
    argv.push_back(nullptr);
    posix_spawn_file_actions_t fa;
    posix_spawn_file_actions_init(&fa);
    posix_spawn_file_actions_addclosefrom_np(&fa, 3);          // the child inherits nothing of the GPU runtime's
    pid_t pid = 0;
    const int rc = posix_spawn(&pid, helper.c_str(), &fa, nullptr, argv.data(), environ);
    posix_spawn_file_actions_destroy(&fa);
    if (rc != 0) {
        cleanup();
        *log = std::string("posix_spawn of sdfk_rtc_helper: ") + strerror(rc);
        return -2;
    }
    // a compiler that never returns (wedged inside comgr, a stale network file system) must not hold its worker thread —
    // and with it sdfk_jit_drain at interpreter exit — for ever: SDFK_RTC_TIMEOUT seconds (default 900), then it is killed
    static const double limit_s = [] { const char* e = getenv("SDFK_RTC_TIMEOUT"); const double v = e ? atof(e) : 0.0; return v > 0.0 ? v : 900.0; }();
    int status = 0;
    bool timed_out = false, cancelled = false;
    const auto t_spawn = std::chrono::steady_clock::now();
    for (;;) {
        const pid_t w = waitpid(pid, &status, WNOHANG);
        if (w == pid) break;
        if (w < 0 && errno != EINTR) { status = -1; break; }
        if (g_cancel_builds.load(std::memory_order_relaxed)) {  // the process is leaving (sdfk_jit_cancel): nobody will use the kernel
            cancelled = true;
            (void)kill(pid, SIGKILL);
            while (waitpid(pid, &status, 0) < 0 && errno == EINTR) {
            }
            break;
        }
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t_spawn).count() > limit_s) {
            timed_out = true;
            (void)kill(pid, SIGKILL);
            while (waitpid(pid, &status, 0) < 0 && errno == EINTR) {
            }
            break;
        }
        std::this_thread::sleep_for(std::chrono::milliseconds(5));
    }
    int result = -1;
    if (cancelled) {
        *log = "build cancelled: the process is shutting down";
    } else if (timed_out) {
        *log = "sdfk_rtc_helper did not finish within " + std::to_string((long long)limit_s) + " s (SDFK_RTC_TIMEOUT) and was killed";
    } else if (WIFEXITED(status) && WEXITSTATUS(status) == 0) {
        FILE* f = fopen(outf.c_str(), "rb");
        if (f && fseek(f, 0, SEEK_END) == 0) {
            const long size = ftell(f);
            if (size > 0 && fseek(f, 0, SEEK_SET) == 0) {
                out->resize((size_t)size);
                if (fread(out->data(), 1, (size_t)size, f) == (size_t)size) result = 0;
            }
        }
        if (f) fclose(f);
        if (result) *log = "sdfk_rtc_helper left no code object";
    } else {
        *log = "sdfk_rtc_helper failed (status " + std::to_string(status) + ")";
        if (FILE* f = fopen((outf + ".log").c_str(), "rb")) {
            char buf[8192];
            const size_t n = fread(buf, 1, sizeof buf - 1, f);
            buf[n] = 0;
            *log += std::string(": ") + buf;
            fclose(f);
        }
    }
    cleanup();
    return result;
}

// *from_disk (optional): the code object came from the on-disk cache
static int rtc_compile(const std::string& src, std::vector<char>* out, std::string* log, int rwb, bool* from_disk = nullptr,
                       std::string* disk_path = nullptr, bool external = false) {
    if (from_disk) *from_disk = false;
    const std::string path = rtc_cache_path(src, rtc_option_key(rwb));
    if (rtc_cache_read(path, out)) {
        if (from_disk) *from_disk = true;
        if (disk_path) *disk_path = path;
        return 0;
    }
    // Builds run in the compiler CHILD process whenever it is there — the background ones (never hiprtc inside this process
    // while the caller is free to dlopen something: profiles/r03_hang_import_during_build.txt) and the ones the caller waits
    // for alike (ctypes releases the GIL during the wait: another Python thread that imports a HIP library would meet the same
    // lock inversion). In-process hiprtc is the last resort, and says so once.
    int rc = -2;
    if (rtc_helper_available()) rc = rtc_compile_external(src, out, log, rwb);
    if (rc == -2 && !external) {
        static std::atomic<bool> told{false};
        if (!told.exchange(true))
            fprintf(stderr, "[sdfk] compiler helper unavailable (%s): building inside this process — do not import HIP libraries on "
                            "other threads meanwhile\n", log->empty() ? "sdfk_rtc_helper not found next to libsdfk.so" : log->c_str());
        std::lock_guard<std::mutex> lk(g_rtc_mu);
        rc = rtc_compile_uncached(src, out, log, rwb);
    }
    if (rc == 0) rtc_cache_write(path, *out);
    return rc;
}

// ---- code objects (per process) and modules (per device) -----------------------------------------
static const char* const kFlavourFn[SDFK_FL_COUNT][2] = {
    {"sdfk_spec_v4", "sdfk_spec_v1"}, {"sdfk_spec_g4", "sdfk_spec_g1"}, {"sdfk_spec_t", nullptr}, {"sdfk_spec_tg", nullptr},
    {"sdfk_spec_tmask", nullptr},     {"sdfk_spec_r", nullptr},         {"sdfk_spec_rg", nullptr}, {"sdfk_spec_rmask", nullptr},
    {"sdfk_spec_r", nullptr},         {"sdfk_spec_rg", nullptr},        {"sdfk_spec_rays", "sdfk_spec_raycam"},
    {"sdfk_spec_occ_list", "sdfk_spec_occ_all"},                        {"sdfk_spec_spans", "sdfk_spec_spancam"},
    {"sdfk_spec_visibility", "sdfk_spec_occlusion"},                    {"sdfk_spec_mom_list", "sdfk_spec_mom_all"}};
// the march flavours: built by the first call that needs them, from programs with or without cull sites, one build each
static bool march_flavour(int f) { return f == SDFK_FL_RAYS || f == SDFK_FL_SPANS || f == SDFK_FL_SECONDARY; }
// ... and the second pair of kernels that long chains get in them (culling along the rays, sdfk_raycull.h): fn[2], fn[3]
static const char* const kMarchCullFn[3][2] = {{"sdfk_spec_rays_cull", "sdfk_spec_raycam_cull"},
                                               {"sdfk_spec_spans_cull", "sdfk_spec_spancam_cull"},
                                               {"sdfk_spec_visibility_cull", "sdfk_spec_occlusion_cull"}};

// hiprtc is entered by ONE thread at a time, and never while a code object is being loaded (hipModuleLoadData):
// g_rtc_mu. Background builds are queued to one worker thread, which is drained before the interpreter / the
// library's statics (and with them hiprtc) go away: sdfk_jit_drain (Python: atexit) and the destructor below.
struct BuildWorker {
    static constexpr int kThreads = 2;                       // compiler processes that may run side by side
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::function<void()>> jobs;
    std::vector<std::thread> threads;
    bool stop = false;
    int busy = 0;
    void post(std::function<void()> job) {
        std::lock_guard<std::mutex> lk(mu);
        jobs.push_back(std::move(job));
        if ((int)threads.size() < kThreads && (int)threads.size() < busy + (int)jobs.size())
            threads.emplace_back([this] { loop(); });
        cv.notify_all();
    }
    void loop() {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [this] { return stop || !jobs.empty(); });
            if (jobs.empty()) return;                        // (stop: the queue is finished first)
            std::function<void()> job = std::move(jobs.front());
            jobs.pop_front();
            ++busy;
            lk.unlock();
            job();
            lk.lock();
            --busy;
            cv.notify_all();
        }
    }
    void drain() {                                           // wait until nothing is queued or running
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [this] { return jobs.empty() && busy == 0; });
    }
    void drop_queued() {
        std::lock_guard<std::mutex> lk(mu);
        jobs.clear();
        cv.notify_all();
    }
    ~BuildWorker() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
            cv.notify_all();
        }
        for (std::thread& t : threads)
            if (t.joinable()) t.join();
    }
};
static BuildWorker g_builds;
extern "C" void sdfk_jit_drain(void) { g_builds.drain(); }
// At interpreter exit: a background build nobody will use any more (a big tree evaluated once: up to a minute of hiprtc)
// must not hold the process. Queued builds are dropped, running compiler children killed, then the workers are idle.
extern "C" void sdfk_jit_cancel(void) {
    g_cancel_builds.store(true);
    g_builds.drop_queued();
    g_builds.drain();
}
static std::atomic<long long> g_compile_count{0};             // hiprtc builds this process has actually run
static std::atomic<long long> g_compile_micros{0};
extern "C" void sdfk_debug_jit_stats(int64_t* builds, double* seconds) {
    if (builds) *builds = g_compile_count.load();
    if (seconds) *seconds = (double)g_compile_micros.load() * 1e-6;
}

static std::shared_ptr<CodeObject> code_entry(const std::string& key) {
    std::lock_guard<std::mutex> lk(g_code_mu);
    std::shared_ptr<CodeObject>& e = g_code[key];
    if (!e) e = std::make_shared<CodeObject>();
    return e;
}
// run one build; the caller has moved the entry to state 1
static void code_build(const std::shared_ptr<CodeObject>& e, const std::string& src, int rwb, bool external = false) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<char> co;
    std::string log;
    bool from_disk = false;
    std::string disk_path;
    const int rc = rtc_compile(src, &co, &log, rwb, &from_disk, &disk_path, external);
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!from_disk) {
        g_compile_count++;
        g_compile_micros += (long long)(dt * 1e6);
    }
    std::lock_guard<std::mutex> lk(e->mu);
    e->build_seconds = dt;
    if (rc == 0) {
        e->co.swap(co);
        e->disk_path = disk_path;
        e->state = 2;
    } else {
        e->error = log;
        e->state = 3;
        e->failed_at = std::chrono::steady_clock::now();
    }
    e->cv.notify_all();
}
// The code object of (source, options): wait = build here (or wait for the thread that is building); !wait = make sure
// a build is under way (background thread) and return at once. A failed build is retried after 30 s at the earliest.
template <typename MakeSource>
static std::shared_ptr<CodeObject> code_get(const std::string& key, MakeSource make_source, int rwb, bool wait) {
    std::shared_ptr<CodeObject> e = code_entry(key);
    std::unique_lock<std::mutex> lk(e->mu);
    if (e->state == 3 && std::chrono::steady_clock::now() - e->failed_at > std::chrono::seconds(30)) e->state = 0;
    if (e->state == 0) {
        e->state = 1;
        lk.unlock();
        const std::string src = make_source();                 // (the program may be gone before a background build ends)
        if (wait || !rtc_helper_available()) {                 // no compiler process to hand the build to: the caller waits
            code_build(e, src, rwb);
        } else {
            g_builds.post([e, src, rwb] { code_build(e, src, rwb, true); });
        }
        return e;
    }
    if (wait) e->cv.wait(lk, [&] { return e->state != 1; });
    return e;
}
// with_flags: the build of a flavour that writes one flag bit per point (value <= threshold) instead of the field — a
// translation unit of its own (#define SDFK_FLAGS), so the field kernels carry none of it.
// with_flags is a set of build VARIANTS: bit 0 = flag-writing build (SDFK_FLAGS), bit 1 = two-row coordinates, z = 0 by
// contract (SDFK_XY: the array kernels never read a third row — sdfk_eval_device_rows2d_xy)
static std::string flavour_key(const sdfk_program* p, int flavour, int rwb, int with_flags = 0) {
    return p->key + "|f" + std::to_string(flavour) + ((with_flags & 1) ? "s" : "") + ((with_flags & 2) ? "x" : "") + "|" + rtc_option_key(rwb);
}
static std::string flavour_source(const sdfk_program* p, int flavour, int with_flags = 0) {
    return std::string((with_flags & 1) ? "#define SDFK_FLAGS 1\n" : "") + ((with_flags & 2) ? "#define SDFK_XY 1\n" : "") +
           sdfk_generate_source(g_ops, SDFK_OP_COUNT, p->code.data(), p->code.size() / 2, p->result_reg, p->sites, flavour,
                                &p->sites_all);
}

extern "C" int sdfk_program_chain_members(const sdfk_program* p) {
    return p && p->chain_mode ? p->chain_members : 0;
}
extern "C" int sdfk_program_compile_check(sdfk_program* p, size_t* code_size) {
    // every flavour this program can be launched with, each as its own translation unit (what a run would build)
    if (!p) return fail(-1, "null program");
    size_t total = 0;
    const int rwb = rows_geo(p);
    for (int f = 0; f < SDFK_FL_COUNT; ++f) {
        if (march_flavour(f)) continue;                         // (not evaluation flavours: built by the first cast / span / secondary call)
        if (f == SDFK_FL_OCCUPANCY) continue;                   // (nor this one: built by the first occupancy call)
        if (f == SDFK_FL_MOMENTS) continue;                     // (nor this one: built by the first moments call)
        if (p->sites.empty() && f != SDFK_FL_PLAIN_ARRAY && f != SDFK_FL_PLAIN_GRID) continue;
        if (p->chain_mode && (f == SDFK_FL_TILE_ARRAY || f == SDFK_FL_TILE_GRID || f == SDFK_FL_TILE_MASK || f == SDFK_FL_ROWS_MASK)) continue;
        std::shared_ptr<CodeObject> e = code_get(flavour_key(p, f, rwb), [&] { return flavour_source(p, f); }, rwb, true);
        if (e->state != 2) return fail(-3, e->error);
        total += e->co.size();
    }
    if (code_size) *code_size = total;
    return 0;
}
/* Build (or fetch) ONE flavour without a GPU: 0 + seconds the build took (0 when it was already there). */
extern "C" int sdfk_program_compile_flavour(sdfk_program* p, int flavour, size_t* code_size, double* seconds) {
    if (!p) return fail(-1, "null program");
    int with_flags = 0;                                                              // build variants (see flavour_key)
    if (flavour >= 0 && (flavour & SDFK_FLAVOUR_FLAGS)) with_flags |= 1;             // the flag-writing build of the flavour
    if (flavour >= 0 && (flavour & SDFK_FLAVOUR_XY)) with_flags |= 2;                // two-row coordinates
    if (flavour >= 0) flavour &= ~(SDFK_FLAVOUR_FLAGS | SDFK_FLAVOUR_XY);
    if (flavour < 0 || flavour >= SDFK_FL_COUNT) return fail(-1, "sdfk_program_compile_flavour: unknown flavour");
    if (p->sites.empty() && flavour != SDFK_FL_PLAIN_ARRAY && flavour != SDFK_FL_PLAIN_GRID && !march_flavour(flavour) &&
        flavour != SDFK_FL_OCCUPANCY && flavour != SDFK_FL_MOMENTS)
        return fail(-2, "sdfk_program_compile_flavour: the program has no cull sites");
    if (with_flags && flavour == SDFK_FL_RAYS)
        return fail(-2, "sdfk_program_compile_flavour: the ray flavour has no flag-writing or two-row build");
    if (with_flags && flavour == SDFK_FL_OCCUPANCY)
        return fail(-2, "sdfk_program_compile_flavour: the occupancy flavour has no flag-writing or two-row build");
    if (with_flags && flavour == SDFK_FL_MOMENTS)
        return fail(-2, "sdfk_program_compile_flavour: the moments flavour has no flag-writing or two-row build");
    if (with_flags && flavour == SDFK_FL_SPANS)
        return fail(-2, "sdfk_program_compile_flavour: the span flavour has no flag-writing or two-row build");
    if (with_flags && flavour == SDFK_FL_SECONDARY)
        return fail(-2, "sdfk_program_compile_flavour: the secondary flavour has no flag-writing or two-row build");
    if ((with_flags & 2) && flavour != SDFK_FL_PLAIN_ARRAY && flavour != SDFK_FL_ROWS2D_ARRAY)
        return fail(-2, "sdfk_program_compile_flavour: two-row coordinates exist for the plain and the flat row-block array kernels");
    if ((with_flags & 1) && (flavour == SDFK_FL_TILE_ARRAY || flavour == SDFK_FL_TILE_GRID || flavour == SDFK_FL_TILE_MASK ||
                       flavour == SDFK_FL_ROWS_MASK))
        return fail(-2, "sdfk_program_compile_flavour: this flavour has no flag-writing build");
    const int rwb = rows_geo(p);
    const auto t0 = std::chrono::steady_clock::now();
    std::shared_ptr<CodeObject> e =
        code_get(flavour_key(p, flavour, rwb, with_flags), [&] { return flavour_source(p, flavour, with_flags); }, rwb, true);
    if (e->state != 2) return fail(-3, e->error);
    if (code_size) *code_size = e->co.size();
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

/* Test aid: build one flavour in the compiler child process (what a background build does), GPU or not. */
extern "C" int sdfk_debug_compile_external(sdfk_program* p, int flavour, size_t* code_size) {
    if (!p) return fail(-1, "null program");
    if (flavour < 0 || flavour >= SDFK_FL_COUNT) return fail(-1, "sdfk_debug_compile_external: unknown flavour");
    if (p->sites.empty() && flavour != SDFK_FL_PLAIN_ARRAY && flavour != SDFK_FL_PLAIN_GRID && !march_flavour(flavour) &&
        flavour != SDFK_FL_OCCUPANCY && flavour != SDFK_FL_MOMENTS)
        return fail(-2, "sdfk_debug_compile_external: the program has no cull sites");
    if (!rtc_helper_available()) return fail(-9, "sdfk_rtc_helper is not next to libsdfk.so (or hiprtc cannot be located)");
    std::vector<char> co;
    std::string log;
    if (rtc_compile_external(flavour_source(p, flavour), &co, &log, rows_geo(p)) != 0) return fail(-3, log);
    if (code_size) *code_size = co.size();
    return 0;
}

// The module of one flavour on one device. wait = false: nullptr while the code object is still being built in the
// background (the caller serves this call from the interpreter kernel — same bits). *err is set on failure.
static std::shared_ptr<SpecModule> get_module(sdfk_program* p, int device, int flavour, bool wait, std::string* err,
                                              int with_flags = 0) {
    const int rwb = rows_geo(p);
    const std::string key = flavour_key(p, flavour, rwb, with_flags);
    std::shared_ptr<SpecModule> m;
    {
        std::lock_guard<std::mutex> lk(g_code_mu);
        std::shared_ptr<SpecModule>& slot = g_mods[std::make_pair(device, key)];
        if (!slot) slot = std::make_shared<SpecModule>();
        m = slot;
    }
    std::lock_guard<std::mutex> lk(m->mu);                     // per (device, flavour): loads never block other devices
    if (m->loaded) return m;
    for (int attempt = 0;; ++attempt) {
        std::shared_ptr<CodeObject> e;
        {
            std::lock_guard<std::mutex> ce(g_code_mu);
            auto it = g_code.find(key);
            if (it != g_code.end()) e = it->second;
        }
        int state = 0;
        if (e) {
            std::lock_guard<std::mutex> el(e->mu);
            state = e->state;
        }
        if (state != 2) {
            e = code_get(key, [&] { return flavour_source(p, flavour, with_flags); }, rwb, wait);
            std::lock_guard<std::mutex> el(e->mu);
            state = e->state;
        }
        if (state == 1) return nullptr;                            // still building (wait == false)
        if (state != 2) {
            std::lock_guard<std::mutex> el(e->mu);
            *err = e->error;
            m->failed = true;
            m->error = e->error;
            return m;                                              // (not marked loaded: a later call asks code_get again)
        }
        hipError_t he;
        {
            std::lock_guard<std::mutex> rl(g_rtc_mu);
            he = hipModuleLoadData(&m->mod, e->co.data());
        }
        for (int i = 0; i < 2 && he == hipSuccess; ++i)
            if (kFlavourFn[flavour][i]) he = hipModuleGetFunction(&m->fn[i], m->mod, kFlavourFn[flavour][i]);
        if (he == hipSuccess && p->chain_mode && !kFlavourFn[flavour][1]) {
            // chain-mode row-block kernels come with the pre-pass of their candidate lists (absent from -DSDFK_NO_CELLS builds)
            const bool grid_fl = flavour == SDFK_FL_ROWS_GRID || flavour == SDFK_FL_ROWS2D_GRID;
            if (hipModuleGetFunction(&m->fn[1], m->mod, grid_fl ? "sdfk_spec_cellsg" : "sdfk_spec_cells") != hipSuccess) {
                m->fn[1] = nullptr;
                (void)hipGetLastError();
            }
        }
        if (he == hipSuccess && march_flavour(flavour)) {
            // long chains come with a second pair of kernels that cull along the rays (SdfkCullField inside the same march)
            const char* const* cull = kMarchCullFn[flavour == SDFK_FL_RAYS ? 0 : flavour == SDFK_FL_SPANS ? 1 : 2];
            if (hipModuleGetFunction(&m->fn[2], m->mod, cull[0]) != hipSuccess ||
                hipModuleGetFunction(&m->fn[3], m->mod, cull[1]) != hipSuccess) {
                m->fn[2] = m->fn[3] = nullptr;
                (void)hipGetLastError();
            }
        }
        if (he == hipSuccess) break;
        // A code object that came from the on-disk cache and does not load (another driver / compiler generation, a
        // damaged file that still passed the checksum): delete the file, forget the blob and build from source once.
        bool retry = false;
        {
            std::lock_guard<std::mutex> el(e->mu);
            if (attempt == 0 && e->state == 2 && !e->disk_path.empty()) {
                (void)remove(e->disk_path.c_str());
                fprintf(stderr, "[sdfk] cached code object %s does not load (%s): rebuilding\n", e->disk_path.c_str(),
                        hipGetErrorString(he));
                e->disk_path.clear();
                e->co.clear();
                e->state = 0;
                retry = true;
            }
        }
        if (m->mod) {
            (void)hipModuleUnload(m->mod);
            m->mod = nullptr;
        }
        (void)hipGetLastError();
        if (retry) {
            wait = true;                                           // the caller gets the rebuilt kernel, not a second failure
            continue;
        }
        m->failed = true;
        m->error = std::string("hipModuleLoadData/GetFunction: ") + hipGetErrorString(he);
        *err = m->error;
        return m;
    }
    m->failed = false;
    m->loaded = true;
    return m;
}

// make sure code / params / tables of `p` are resident on the current device
static int ensure_resident(sdfk_program* p, int device, hipStream_t stream, DevState** out) {
    std::lock_guard<std::mutex> lk(p->mu);
    DevState& d = p->dev[device];
    if (!d.d_code) {
        HIPCHK(hipMalloc(&d.d_code, p->code.size() * sizeof(uint32_t)));
        HIPCHK(hipMemcpy(d.d_code, p->code.data(), p->code.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIPCHK(hipMalloc(&d.d_params, std::max<size_t>(p->params.size(), 1) * sizeof(float)));
        HIPCHK(hipMalloc(&d.d_tables, std::max<size_t>(p->tables.size(), 1) * sizeof(float)));
        if (!p->tables.empty())
            HIPCHK(hipMemcpy(d.d_tables, p->tables.data(), p->tables.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (d.params_version != p->params_version) {
        // enqueued on the caller's stream (it must not overtake kernels of that stream that still read the old values)
        // and WAITED for: other streams of the device (the two slots of the host pipeline) launch right after this
        if (!p->params.empty()) {
            HIPCHK(hipMemcpyAsync(d.d_params, p->params.data(), p->params.size() * sizeof(float),
                                  hipMemcpyHostToDevice, stream));
            HIPCHK(hipStreamSynchronize(stream));
        }
        d.params_version = p->params_version;
    }
    *out = &d;
    return 0;
}
