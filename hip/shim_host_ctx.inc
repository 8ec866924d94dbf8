// shim_host_ctx.inc -- per-thread host-side state of the shim (included inside cute_nt.hip's anonymous namespace):
// the staging-copy pool, the per-device context (streams, grow-only device scratch, pinned staging, events) and the
// helpers of the host tier that are not part of its pipeline.
#include "copy_pool.hpp"

// ---- FRESH outputs ------------------------------------------------------------------------
// The reference's functions return a new Vec, so the drop-in's copy-out usually lands in pages that do not exist yet
// and every first touch is a page fault (a 1-GiB decode: 79 ms into a fresh buffer against 26 ms into a warm one,
// BENCH_r02 host_tier).  What helps, measured on the GPU box (bench/host_fresh_lab.py, 1-GiB decode, output allocated
// inside the call and dropped outside the timed loop; 22.8 ms into a warm buffer):
//   MADV_HUGEPAGE on the output (advise_huge_output below): the faults, and the caller's later free(), in 2-MiB units;
//   the copy-out of a fresh output uses the WHOLE copy pool (CopyPool::copy fresh_pages = true), in 2-MiB blocks cut on
//     the OUTPUT's 2-MiB grid so that every transparent huge page is faulted in by exactly one thread: 35 -> 23-24 ms =
//     1.04-1.08x the warm call for both directions (with unaligned 2-MiB slices, eight threads fighting over the same
//     huge pages: 27-33 ms; profiles/r03_host_copy_blocks.jsonl);
//   a separate team of helper threads touching the pages AHEAD of the copy-out (an atomic add-0 per page) was built
//     and measured too: worth 0-5 % on top of four copy threads, and WORSE than nothing once the copy-out itself uses
//     eight (31.0 vs 27.3 ms: the helpers' zeroed lines sit dirty in other cores' caches) -- removed;
//   MADV_POPULATE_WRITE: slower than touching under THP (bench/fresh_pages_lab.cpp).
// What a caller that ALSO drops its previous result inside its timed loop sees on top is the host kernel's munmap --
// 47 ms per GiB of huge pages, 120 ms per GiB of 4-KiB pages on that box, with or without a HIP runtime in the process
// (bench/munmap_lab.cpp); the reference's own functions pay it just the same, and the huge-page advice is what brings
// it from 120 to 47.
// "Fresh" = more than half of 16 sample pages spread over the buffer are not resident (mincore).
inline bool output_is_fresh(void* p, size_t bytes) {
    if (bytes < ((size_t)8 << 20)) return false;
    const uintptr_t page = 4096;
    const uintptr_t lo = (reinterpret_cast<uintptr_t>(p) + page - 1) & ~(page - 1);
    const uintptr_t hi = (reinterpret_cast<uintptr_t>(p) + bytes) & ~(page - 1);
    if (hi <= lo) return false;
    int absent = 0, seen = 0;
    for (int k = 0; k < 16; ++k) {
        const uintptr_t a = lo + ((hi - lo) / page * (uintptr_t)k / 16) * page;
        unsigned char vec = 0;
        if (mincore(reinterpret_cast<void*>(a), page, &vec) == 0) {
            ++seen;
            absent += !(vec & 1);
        }
    }
    return seen > 0 && 2 * absent > seen;
}

// CPUs of the NUMA node a device sits on (empty set = unknown / not pinning)
struct NumaInfo {
    int node = -1;
    int n_cpus = 0;
    cpu_set_t cpus;
    char bdf[32] = {0};
};

bool parse_cpulist(const char* text, cpu_set_t* out) {  // "0-63,128-191"
    CPU_ZERO(out);
    const char* p = text;
    bool any = false;
    while (*p) {
        char* end = nullptr;
        long lo = strtol(p, &end, 10);
        if (end == p) break;
        long hi = lo;
        p = end;
        if (*p == '-') {
            hi = strtol(p + 1, &end, 10);
            if (end == p + 1) break;
            p = end;
        }
        for (long c = lo; c <= hi && c < CPU_SETSIZE; ++c) {
            if (c >= 0) {
                CPU_SET((int)c, out);
                any = true;
            }
        }
        while (*p == ',' || *p == ' ' || *p == '\n') ++p;
    }
    return any;
}

bool read_small_file(const char* path, char* buf, size_t cap) {
    FILE* f = fopen(path, "r");
    if (!f) return false;
    const size_t n = fread(buf, 1, cap - 1, f);
    fclose(f);
    buf[n] = 0;
    return n > 0;
}

NumaInfo numa_of_device(int device, const cpu_set_t& allowed) {
    NumaInfo info;
    CPU_ZERO(&info.cpus);
    if (hipDeviceGetPCIBusId(info.bdf, (int)sizeof info.bdf, device) != hipSuccess) {
        (void)hipGetLastError();
        info.bdf[0] = 0;
        return info;
    }
    for (char* c = info.bdf; *c; ++c)
        if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');  // sysfs spells the address in lower case
    char path[160], buf[4096];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", info.bdf);
    if (!read_small_file(path, buf, sizeof buf)) return info;
    const int node = atoi(buf);
    if (node < 0) return info;  // -1: the platform does not say
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    cpu_set_t node_cpus;
    if (!read_small_file(path, buf, sizeof buf) || !parse_cpulist(buf, &node_cpus)) return info;
    CPU_AND(&info.cpus, &node_cpus, &allowed);
    info.n_cpus = CPU_COUNT(&info.cpus);
    info.node = node;
    return info;
}


// ---- NUMA placement of the single-GPU host tier (round 6) -------------------------------------
// The sharded tier pins its workers to their GPU's node; the single-GPU tier used to leave everything where the caller
// happened to be.  Now, per calling thread and device, the GPU's node is read once (sysfs, numa_of_device), the pinned staging
// ring is allocated from a short-lived thread pinned to that node's CPUs and the copy team's HELPERS are pinned there, one per
// L3 domain (CCD) -- the caller itself is never moved.  CNT_HOST_NUMA=0 switches all of it off.  What it buys, measured
// (profiles/r06_host_tier.md 2-3): hipHostMalloc puts the ring on the GPU's node by itself, whoever calls it; one helper per
// CCD is a guard against the 60-GB/s-per-CCD ceiling, not a gain over the scheduler's usual placement; and a caller THREAD on
// the far socket is within 1 % of a near one either way -- the far-socket losses of rounds 3-5 were the copy-engine binding
// that DevCtx::warm_copy_engines now fixes.  A whole PROCESS confined to the far socket still loses 8 % on decode.
inline bool host_numa_enabled() {
    static const bool on = [] {
        const char* e = getenv("CNT_HOST_NUMA");
        return !(e && e[0] == '0');
    }();
    return on;
}
// The last-level-cache domains (CCDs) of a CPU set, in CPU order: /sys/devices/system/cpu/cpuN/cache/index3/shared_cpu_list names
// each CPU's; a domain is kept as its intersection with `cpus`.  One read per CPU, once per calling thread and device.
inline std::vector<cpu_set_t> l3_domains_of(const cpu_set_t& cpus) {
    std::vector<cpu_set_t> out;
    cpu_set_t seen;
    CPU_ZERO(&seen);
    for (int c = 0; c < CPU_SETSIZE; ++c) {
        if (!CPU_ISSET(c, &cpus) || CPU_ISSET(c, &seen)) continue;
        char path[128], buf[4096];
        cpu_set_t dom;
        snprintf(path, sizeof path, "/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list", c);
        if (!read_small_file(path, buf, sizeof buf) || !parse_cpulist(buf, &dom)) {
            CPU_ZERO(&dom);
            CPU_SET(c, &dom);  // no L3 description: the CPU is a domain of its own kind -- folded into one set below
        }
        CPU_AND(&dom, &dom, &cpus);
        CPU_SET(c, &dom);
        CPU_OR(&seen, &seen, &dom);
        out.push_back(dom);
    }
    if (out.size() > 64) {  // no usable cache topology (every CPU on its own): one domain, the whole set
        out.assign(1, cpus);
    }
    return out;
}

constexpr bool kHostWarmDefault = true;       // DevCtx::warm_copy_engines
constexpr bool kHostPreallocDefault = true;   // host_tier.inc host_prealloc

// node of the page at p (move_pages with a NULL target list only asks): -1 = the kernel does not say (not a page it migrates:
// device-mapped pinned memory answers that on some drivers)
inline int numa_node_of_page(const void* p) {
    if (!p) return -1;
    void* page = reinterpret_cast<void*>(reinterpret_cast<uintptr_t>(p) & ~(uintptr_t)4095);
    int status = -1;
    if (syscall(SYS_move_pages, 0, 1UL, &page, nullptr, &status, 0) != 0) return -1;
    return status >= 0 ? status : -1;
}

// ---- per-thread device context (streams + grow-only device scratch + pinned staging) ----
// Slots of the host tier's pipeline (stream + pinned staging + device scratch each).  Not two: with two the H2D
// engine idles while the host retires and restages the slot it has just finished, and both directions of the link are
// never busy at once.  Four since round 6 (three from round 3 on): with 8-Mi-nt chunks and the copy engines warmed the
// fourth is worth 2-4 % at 2^26-2^30 nt and 7-20 % at 2^21-2^24 (profiles/r06_host_tier.md 8; CNT_HOST_SLOTS = 2..4 for A/B).
constexpr int kMaxSlots = 4;
constexpr int kHostSlotsDefault = 4;
inline int host_slots() {
    static const int v = [] {
        const char* e = getenv("CNT_HOST_SLOTS");
        const int n = e ? atoi(e) : kHostSlotsDefault;
        return n < 2 ? 2 : n > kMaxSlots ? kMaxSlots : n;
    }();
    return v;
}

// Is [p, p + bytes) pinned host memory the copy engines can use in place -- hipHostMalloc'ed (cnt_host_alloc, a torch tensor
// with pin_memory=True ...) or hipHostRegister'ed (cnt_host_register)?  Then the host tier skips its staging copy on that side
// (host_tier.inc): the DMA reads / writes the caller's buffer itself.  Two or three runtime queries (~1 us); ordinary memory
// makes the first one fail, which is the answer.  The range must lie inside ONE allocation or ONE registration: a range that
// runs from one registration into the next (adjacent or not), over an unregistered hole or out of pinned memory is staged,
// whatever its two ends are.  hipMemGetAddressRange gives a hipHostMalloc'ed allocation's base and size; for registered memory
// it gives the registration's size but no base (ROCm 7.2), and HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, asked at p, supplies the
// registration's first byte (the same answer at every byte of it; devicePointer is p's own device address, not the
// registration's).  No answer from either: staged.  CNT_HOST_PINNED=0: never look, always stage.
inline bool host_pinned_enabled() {
    static const bool v = [] {
        const char* e = getenv("CNT_HOST_PINNED");
        return !(e && e[0] == '0');
    }();
    return v;
}
inline bool pinned_host_byte(const void* p, hipPointerAttribute_t* a) {
    if (hipPointerGetAttributes(a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a->type == hipMemoryTypeHost;
}
inline bool host_range_in_one_pinned(const void* p, size_t bytes, void** device_view) {
    if (!p || !bytes) return false;
    hipPointerAttribute_t a;
    if (!pinned_host_byte(p, &a)) return false;
    if (device_view) *device_view = a.devicePointer;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    const void* dp = a.devicePointer ? a.devicePointer : p;
    const hipError_t ranged = hipMemGetAddressRange(&base, &size, const_cast<void*>(dp));
    if (ranged == hipSuccess && base) {  // hipHostMalloc'ed: the allocation's base and size
        const uintptr_t lo = reinterpret_cast<uintptr_t>(dp), end = reinterpret_cast<uintptr_t>(base) + size;
        return lo + bytes >= lo && lo + bytes <= end;
    }
    if (ranged != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    // registered in place: the registration that holds p starts at `start` (asked with p: an address of p's space) and is
    // `size` bytes long; the range must end inside it
    void* start = nullptr;
    if (hipPointerGetAttribute(&start, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, const_cast<void*>(p)) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p), first = reinterpret_cast<uintptr_t>(start);
    return start && size && first <= lo && lo - first <= size && bytes <= size - (lo - first);
}
inline bool host_range_is_pinned(const void* p, size_t bytes, void** device_view = nullptr /* how a kernel addresses p */) {
    return host_pinned_enabled() && host_range_in_one_pinned(p, bytes, device_view);
}
// Does [p, p + bytes) start in pinned memory and leave it (into ordinary memory, another registration, past a hole)?  The
// runtime then refuses a hipMemcpy* of the range (hipErrorInvalidValue, ROCm 7.2: it holds the copy to the allocation or
// registration of its first byte), so a staged copy of it has to go through ordinary memory (host_call's bounce buffers).
inline bool host_range_leaves_pinned(const void* p, size_t bytes) {
    hipPointerAttribute_t a;
    return p && bytes && pinned_host_byte(p, &a) && !host_range_in_one_pinned(p, bytes, nullptr);
}

struct DevCtx {
    int device = -1;
    hipStream_t stream[kMaxSlots] = {nullptr, nullptr, nullptr, nullptr};
    void* d_in[kMaxSlots] = {nullptr, nullptr, nullptr, nullptr};
    void* d_out[kMaxSlots] = {nullptr, nullptr, nullptr, nullptr};
    uint8_t* h_in[kMaxSlots] = {nullptr, nullptr, nullptr, nullptr};   // pinned
    uint8_t* h_out[kMaxSlots] = {nullptr, nullptr, nullptr, nullptr};  // pinned
    void* hd_in = nullptr;   // h_in[0] / h_out[0] as the device sees them (zero-copy path for small inputs)
    void* hd_out = nullptr;
    size_t cap_in = 0, cap_out = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};  // device-resident sharded tier: per-shard kernel time
    void* d_aux[3] = {nullptr, nullptr, nullptr};  // device-only grow-only scratch of the packed-ops host tier (no pinned twin)
    size_t cap_aux[3] = {0, 0, 0};
    uint32_t* h_flag = nullptr;  // pinned completion word of the small-call path, and how the device sees it
    void* hd_flag = nullptr;
    uint32_t tick = 0;
    NumaInfo numa;            // of this device, against the mask the calling thread had when it first came here
    bool numa_asked = false;
    std::vector<cpu_set_t> copy_domains;  // where the copy team's helpers go: the L3 domains of the GPU's node -- of the caller's whole
                                          // mask when that excludes the node (a process under `taskset` stays inside its mask)

    void ask_numa() {
        if (numa_asked) return;
        numa_asked = true;
        cpu_set_t allowed;
        CPU_ZERO(&allowed);
        if (sched_getaffinity(0, sizeof allowed, &allowed) != 0)
            for (int c = 0; c < CPU_SETSIZE; ++c) CPU_SET(c, &allowed);
        numa = numa_of_device(device, allowed);
        copy_domains = l3_domains_of(numa.n_cpus > 0 ? numa.cpus : allowed);
    }
    // the domain the helpers start behind: the one after the caller's own (the caller copies too), else one that depends on
    // which pool this is, so that several calling threads do not stack their helpers on the same CCDs
    size_t first_copy_domain(size_t pool_id) const {
        const int cpu = sched_getcpu();
        for (size_t i = 0; cpu >= 0 && cpu < CPU_SETSIZE && i < copy_domains.size(); ++i)
            if (CPU_ISSET(cpu, &copy_domains[i])) return i + 1;
        return pool_id * 3;
    }
    // f() on a short-lived thread pinned to the CPUs of this device's NUMA node (with this device current there): host memory
    // it allocates or first touches is placed under that node's local policy.  Directly on the caller when placement is off,
    // the node is unknown, or the caller is running on that node already.
    template <typename F>
    int on_gpu_node(F&& f) {
        ask_numa();
        const int cpu = sched_getcpu();
        if (!host_numa_enabled() || numa.n_cpus == 0 || (cpu >= 0 && cpu < CPU_SETSIZE && CPU_ISSET(cpu, &numa.cpus))) return f();
        int rc = CNT_OK;
        std::thread t([&] {
            (void)pthread_setaffinity_np(pthread_self(), sizeof numa.cpus, &numa.cpus);
            rc = hip_rc(hipSetDevice(device));
            if (rc == CNT_OK) rc = f();
        });
        t.join();
        return rc;
    }

    int ensure_streams() {
        for (int i = 0; i < host_slots(); ++i)
            if (!stream[i]) HIP_TRY(hipStreamCreateWithFlags(&stream[i], hipStreamNonBlocking));
        return CNT_OK;
    }
    int ensure_events() {
        for (int i = 0; i < 2; ++i)
            if (!ev[i]) HIP_TRY(hipEventCreate(&ev[i]));
        return CNT_OK;
    }
    int ensure_aux(int i, size_t bytes) {
        CNT_TRY(ensure_streams());
        if (bytes > cap_aux[i]) {
            cap_aux[i] = 0;
            void* old = d_aux[i];
            d_aux[i] = nullptr;  // cleared first: a failing hipFree must not leave a pointer behind that is freed again later
            if (old) HIP_TRY(hipFree(old));
            HIP_TRY(hipMalloc(&d_aux[i], bytes));
            cap_aux[i] = bytes;
        }
        return CNT_OK;
    }
    int ensure(size_t need_in, size_t need_out) {
        if (need_in <= cap_in && need_out <= cap_out && h_flag && stream[0]) return CNT_OK;
        return on_gpu_node([&] { return ensure_here(need_in, need_out); });
    }
    int ensure_here(size_t need_in, size_t need_out) {
        CNT_TRY(ensure_streams());
        if (!h_flag) {
            HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_flag), 64, hipHostMallocDefault));
            *h_flag = 0;
            HIP_TRY(hipHostGetDevicePointer(&hd_flag, h_flag, 0));
        }
        if (need_in > cap_in) {
            cap_in = 0;  // a failure below must not leave a stale capacity behind
            for (int i = 0; i < host_slots(); ++i) {
                void* old_d = d_in[i];
                uint8_t* old_h = h_in[i];
                d_in[i] = nullptr;  // cleared first, see ensure_aux
                h_in[i] = nullptr;
                if (old_d) HIP_TRY(hipFree(old_d));
                if (old_h) HIP_TRY(hipHostFree(old_h));
                HIP_TRY(hipMalloc(&d_in[i], need_in));
                HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_in[i]), need_in, hipHostMallocDefault));
            }
            HIP_TRY(hipHostGetDevicePointer(&hd_in, h_in[0], 0));
            cap_in = need_in;
        }
        if (need_out > cap_out) {
            cap_out = 0;
            for (int i = 0; i < host_slots(); ++i) {
                void* old_d = d_out[i];
                uint8_t* old_h = h_out[i];
                d_out[i] = nullptr;
                h_out[i] = nullptr;
                if (old_d) HIP_TRY(hipFree(old_d));
                if (old_h) HIP_TRY(hipHostFree(old_h));
                HIP_TRY(hipMalloc(&d_out[i], need_out));
                HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_out[i]), need_out, hipHostMallocDefault));
            }
            HIP_TRY(hipHostGetDevicePointer(&hd_out, h_out[0], 0));
            cap_out = need_out;
        }
        if (!engines_warmed && cap_in >= kWarmBytes && cap_out >= kWarmBytes) CNT_TRY(warm_copy_engines());
        return CNT_OK;
    }
    // The runtime binds a stream to a copy (SDMA) engine when the stream FIRST copies, and takes the engines that are idle at
    // that moment: streams whose first copies do not overlap in time all get the same engine and serialise on it for the rest
    // of the process -- which is what a thread's first pipelined call being a small one did (1-MiB chunks, 20 us each, the copy
    // team still starting up between them): every later call of the process 15-20 % slower, 25.9 instead of 22.1 ms per GiB,
    // deterministically (bench/host_tier_lab.py history, profiles/r06_host_tier.md).  So the ring's streams make their first
    // copies HERE, once, long ones, all slots at the same time and both directions at the same time.
    static constexpr size_t kWarmBytes = (size_t)4 << 20;  // above anything a zero-copy call stages: only a pipelined call's ring is warmed
    bool engines_warmed = false;
    int warm_copy_engines() {
        static const bool on = [] {
            const char* e = getenv("CNT_HOST_WARM");
            return e ? e[0] != '0' : kHostWarmDefault;
        }();
        engines_warmed = true;
        if (!on) return CNT_OK;
        const size_t n_in = std::min(cap_in, (size_t)16 << 20), n_out = std::min(cap_out, (size_t)16 << 20);
        int rc = CNT_OK;
        for (int rep = 0; rep < 2 && rc == CNT_OK; ++rep) {
            for (int i = 0; i < host_slots() && rc == CNT_OK; ++i) rc = hip_rc(hipMemcpyAsync(d_in[i], h_in[i], n_in, hipMemcpyHostToDevice, stream[i]));
            for (int i = 0; i < host_slots() && rc == CNT_OK; ++i) rc = hip_rc(hipMemcpyAsync(h_out[i], d_out[i], n_out, hipMemcpyDeviceToHost, stream[i]));
        }
        for (int i = 0; i < host_slots(); ++i) {
            const int r2 = hip_rc(hipStreamSynchronize(stream[i]));
            if (rc == CNT_OK) rc = r2;
        }
        return rc;
    }
    void release() {
        if (device < 0) return;
        int prev = -1;
        (void)hipGetDevice(&prev);
        if (hipSetDevice(device) == hipSuccess) {
            for (int k = 0; k < 3; ++k) {
                if (d_aux[k]) (void)hipFree(d_aux[k]);
                d_aux[k] = nullptr;
                cap_aux[k] = 0;
            }
            if (h_flag) {
                (void)hipHostFree(h_flag);
                h_flag = nullptr;
                hd_flag = nullptr;
            }
            for (int i = 0; i < 2; ++i) {
                if (ev[i]) (void)hipEventDestroy(ev[i]);
                ev[i] = nullptr;
            }
            for (int i = 0; i < kMaxSlots; ++i) {
                if (stream[i]) (void)hipStreamDestroy(stream[i]);
                if (d_in[i]) (void)hipFree(d_in[i]);
                if (d_out[i]) (void)hipFree(d_out[i]);
                if (h_in[i]) (void)hipHostFree(h_in[i]);
                if (h_out[i]) (void)hipHostFree(h_out[i]);
                stream[i] = nullptr;
                d_in[i] = d_out[i] = nullptr;
                h_in[i] = h_out[i] = nullptr;
            }
        }
        cap_in = cap_out = 0;
        engines_warmed = false;  // the streams are gone: new ones bind anew
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

inline size_t next_pool_id() {
    static std::atomic<size_t> n{0};
    return n.fetch_add(1, std::memory_order_relaxed);
}
struct ThreadCtx {
    std::map<int, DevCtx> per_device;
    CopyPool pool;
    size_t pool_id = next_pool_id();
    int placed_device = -1;  // the device whose node the helpers were last placed by
    ~ThreadCtx() {
        pool.stop();
        for (auto& kv : per_device) kv.second.release();
    }
    int get(DevCtx** out) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e == hipErrorNoDevice ? CNT_ENODEV : hip_rc(e);
        DevCtx& c = per_device[dev];
        c.device = dev;
        *out = &c;
        // the copy team's helpers follow the device the calling thread works on (CNT_HOST_NUMA, above): one CCD each.  The
        // first domain is fixed when the placement is first made for this pool -- a caller that migrates does not restart its team.
        c.ask_numa();
        if (!host_numa_enabled()) {
            pool.set_domains({}, 0);
        } else if (placed_device != dev) {
            placed_device = dev;
            pool.set_domains(c.copy_domains, c.first_copy_domain(pool_id));
        }
        return CNT_OK;
    }
};
thread_local ThreadCtx t_ctx;

// Host-tier chunking: 8 Mi nucleotides per chunk = ~0.15 ms of PCIe time per chunk (round 6, bench/host_tier_lab.py pipeline,
// profiles/r06_host_tier.md: against 16 Mi the 2^26 ... 2^28-nt calls gain 2-4 % -- fill and drain are one chunk's worth of
// un-overlapped work -- and 1-GiB calls are unchanged; 4 Mi loses 15 % everywhere to the per-chunk host cost).  Footprint per
// calling thread (and per sharded-tier worker) and device: slots x (chunk + chunk) of pinned staging and as much device scratch --
// at the default 4 slots 4 x (8 + 8) MiB = 64 MiB pinned + 64 MiB of HBM, allocated WHOLE by the thread's first pipelined call
// (> 2^20 nt) so that the ring's streams can make their first copies long and simultaneous (DevCtx::warm_copy_engines);
// cnt_shutdown() releases the calling thread's share.
#ifndef CNT_CHUNK_MI
#define CNT_CHUNK_MI 8  // build-time default; CNT_HOST_CHUNK_MI overrides it at run time for A/B runs
#endif
constexpr int kSmallDirectMaxLog2 = 25;   // both sides pinned: up to 2^this nt ONE kernel reads / writes the caller's buffers over the link
constexpr int kDirectRampLog2 = 25;       // calls with BOTH sides pinned: ramped pieces from 2^25 nt, two slots of equal pieces below
constexpr int kHostRampLog2Default = 0;  // calls of >= 2^this nt ramp their piece sizes up and down (host_tier.inc Pieces); 0 = never
constexpr int kHostNtDefault = 0;    // which of the pipeline's copies use non-temporal stores (host_tier.inc host_nt)
constexpr int kPipelinePieces = 4;  // mid-size calls are cut into at least this many chunks (host_tier.inc pipeline_chunk)
constexpr size_t kChunkNt = (size_t)CNT_CHUNK_MI << 20;       // multiple of 32
constexpr size_t kChunkNt5 = (size_t)27 * (CNT_CHUNK_MI * 32) << 10;  // 27-nt words: 256 Ki words per chunk (6.75 Mi nt) at the default

// Small host-tier calls skip the two DMA submissions: the kernels read the pinned staging buffer and
// write the pinned result buffer directly over PCIe (zero-copy), so a call is memcpy, one launch, one
// stream sync, memcpy.  CNT_ZEROCOPY_MAX_NT overrides the size limit (0 disables the path).
// ... and when BOTH of a call's slices are pinned, the kernel reads and writes the CALLER's buffers over the link: no memcpy on
// either side, no copy engine.  2^20 nt: 64 / 75 us -> 36 / 33; the kernel pulls its input at 49-54 GB/s, the link's rate, and
// writes while it reads, so it beats the pinned pipeline up to 2^25 nt (2^22: 141 / 144 -> 113 / 103 us; 2^24: 405 / 427 -> 387 /
// 365; 2^25: 770 / 765 -> 691 / 676) and ties with it at 2^26-2^27 (profiles/r06_host_tier.md 9).  From CNT_DIRECT_MIN_NT (2^16:
// below, the copies cost less than asking the runtime about two pointers) up to CNT_DIRECT_MAX_NT (2^25).
size_t small_direct_min_nt() {
    static const size_t v = [] {
        const char* e = getenv("CNT_DIRECT_MIN_NT");
        return e ? (size_t)strtoull(e, nullptr, 10) : (size_t)1 << 16;
    }();
    return v;
}
size_t small_direct_max_nt() {
    static const size_t v = [] {
        const char* e = getenv("CNT_DIRECT_MAX_NT");
        return e ? (size_t)strtoull(e, nullptr, 10) : (size_t)1 << kSmallDirectMaxLog2;
    }();
    return v;
}
size_t zero_copy_max_nt(bool decode = false) {
    static const size_t env = [] {
        const char* e = getenv("CNT_ZEROCOPY_MAX_NT");
        return e ? (size_t)strtoull(e, nullptr, 10) : SIZE_MAX;
    }();
    if (env != SIZE_MAX) return env;
    // round 6 (four slots, 8-Mi chunks): the single kernel still wins at 2^21 nt for the encode (114 against 119 us) and up to 2^22
    // for the decode (204 against 224-230), and loses above (profiles/r06_host_tier.md 11)
    return (size_t)1 << (decode ? 22 : 21);
}

// End of a small (zero-copy) host-tier call: instead of hipStreamSynchronize, a one-thread kernel behind the
// codec kernel raises a pinned word and the host spins on it -- the call's results are in pinned memory that
// the kernel has released to system scope by then.  bench/latency_lab.hip, 40 000 nt: 18.8 us with the
// stream sync, 15.5 us with the flag (12.0 us together with the 16-B-load staged kernel; an empty launch +
// sync is 11.1 us).  Anything slower than ~200 us, and any failure, falls back to the blocking sync, which
// also collects the error.  CNT_HOST_SPIN=0 always uses the sync.
int finish_small_call(DevCtx* c, hipStream_t s) {
    static const bool spin = [] {
        const char* e = getenv("CNT_HOST_SPIN");
        return !(e && e[0] == '0');
    }();
    if (spin && c->hd_flag) {
        const uint32_t t = ++c->tick;
        hipLaunchKernelGGL(raise_flag, dim3(1), dim3(1), 0, s, static_cast<uint32_t*>(c->hd_flag), t);
        if (hipGetLastError() == hipSuccess) {
            const auto t0 = std::chrono::steady_clock::now();
            for (unsigned spins = 1;; ++spins) {
                if (__atomic_load_n(c->h_flag, __ATOMIC_ACQUIRE) == t) return CNT_OK;
#if defined(__x86_64__)
                __builtin_ia32_pause();
#endif
                if ((spins & 255u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(200)) break;
            }
        }
    }
    return hip_rc(hipStreamSynchronize(s));
}

// madvise(MADV_HUGEPAGE) on those 2-MiB units of a large output whose pages DO NOT EXIST YET, so that their first touches
// -- and, later, the caller's free() -- work in 2-MiB units where transparent huge pages are in `madvise` mode (the GPU
// box, most distributions).  ON by default, CNT_HOST_HUGEPAGE=0 switches it off.  It is the one thing the library does to
// caller memory besides writing the result, and since round 4 it is scoped: one mincore() walk over the output's
// 2-MiB-aligned interior finds the maximal runs of units in which NO page is resident, and only those runs are advised.
// A warm output (a reused buffer, the `_into` forms, a Vec the caller has already written) is never advised: its VMA
// flags, its layout and its RSS stay exactly as the caller made them (tests/test_hugepage_scope.py reads
// /proc/self/smaps before and after).  A fresh malloc / Vec::with_capacity / np.empty is advised as before -- that is
// where the advice pays: 1-GiB decode into a fresh malloc freed inside the timed loop 150 ms per call without it, 72-91 ms
// with it (munmap of 1 GiB: 120 ms in 4-KiB pages, 47 ms in huge pages on that host, bench/munmap_lab.cpp;
// profiles/r03_bench_twin.log vs r03_bench_twin_no_advice.log); numpy advises its own large allocations, nothing either
// way there (profiles/r03_host_fresh_final.jsonl).  The walk costs ~0.2 ms per GiB against a 22-ms call.
void advise_huge_output(void* out, size_t bytes) {
    static const bool on = [] {
        const char* e = getenv("CNT_HOST_HUGEPAGE");
        return !(e && e[0] == '0');
    }();
    constexpr uintptr_t kHuge = (uintptr_t)2 << 20, kPage = 4096, kPagesPerHuge = kHuge / kPage;
    if (!on || bytes < 4 * kHuge) return;
    const uintptr_t lo = (reinterpret_cast<uintptr_t>(out) + kHuge - 1) & ~(kHuge - 1);
    const uintptr_t hi = (reinterpret_cast<uintptr_t>(out) + bytes) & ~(kHuge - 1);
    if (hi <= lo) return;
    constexpr size_t kUnitsPerWalk = 32;  // 64 MiB per mincore call: a 16-KiB residency vector on the stack
    unsigned char vec[kUnitsPerWalk * kPagesPerHuge];
    uintptr_t run_lo = 0;  // start of the current run of wholly absent units (0 = none open)
    auto close_run = [&](uintptr_t end) {
        if (run_lo && end > run_lo) (void)madvise(reinterpret_cast<void*>(run_lo), end - run_lo, MADV_HUGEPAGE);
        run_lo = 0;
    };
    for (uintptr_t a = lo; a < hi; a += kUnitsPerWalk * kHuge) {
        const size_t units = std::min<size_t>(kUnitsPerWalk, (hi - a) / kHuge);
        if (mincore(reinterpret_cast<void*>(a), units * kHuge, vec) != 0) {  // not a mapping we can read: leave it alone
            close_run(a);
            continue;
        }
        for (size_t u = 0; u < units; ++u) {
            bool any = false;
            for (size_t p = 0; p < kPagesPerHuge && !any; ++p) any = (vec[u * kPagesPerHuge + p] & 1) != 0;
            if (any) close_run(a + u * kHuge);
            else if (!run_lo) run_lo = a + u * kHuge;
        }
    }
    close_run(hi);
}
