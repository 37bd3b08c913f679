// Small helper kernels around the implicit-GEMM cores: weight packing, split-K
// slab reduction, per-channel sums.
#include <string.h>

#include <atomic>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "igemm_host.h"

namespace cnuda {
namespace {

__global__ void pack_kernel(const float* __restrict__ W, float* __restrict__ dst, int Co, int C, int T,
                            int mode, int Kp, int Mp, int Cpad) {
    const long long total = (long long)Kp * Mp;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(i / Mp), m = (int)(i % Mp);
        int o = -1, c = -1, tap = -1;
        if (mode == PACK_FWD) {
            if (k < T * C && m < Co) { tap = k / C; c = k % C; o = m; }
        } else if (mode == PACK_HALO_FWD) {
            if (k < T * C && m < Co) { const int g = k / (16 * T), r = k - g * 16 * T; tap = r >> 4; c = 16 * g + (r & 15); o = m; }
        } else if (mode == PACK_HALO_DGRAD) {
            if (k < T * Co && m < C) { const int g = k / (16 * T), r = k - g * 16 * T; tap = T - 1 - (r >> 4); o = 16 * g + (r & 15); c = m; }
        } else {   // PACK_DGRAD: Cpad = Co rounded up to the K chunk, rows o >= Co stay zero
            if (k < T * Cpad && m < C) { tap = k / Cpad; o = k % Cpad; c = m; if (o >= Co) o = -1; }
        }
        dst[i] = (o >= 0) ? W[((size_t)o * C + c) * T + tap] : 0.0f;
    }
}

struct TapList { int n; int tap[9]; };
// dst[k = ti*Co + o][m = c] = W[o][c][taps.tap[ti]]   (transposed-conv operand restricted to a tap subset)
__global__ void pack_taps_kernel(const float* __restrict__ W, float* __restrict__ dst, int Co, int C, int T,
                                 TapList taps, int Kp, int Mp) {
    const long long total = (long long)Kp * Mp;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(i / Mp), m = (int)(i % Mp);
        float v = 0.0f;
        if (k < taps.n * Co && m < C) {
            const int ti = k / Co, o = k - ti * Co;
            v = W[((size_t)o * C + m) * T + taps.tap[ti]];
        }
        dst[i] = v;
    }
}

// The same sum for Z <= 4 slabs, one thread per output: ((s0 + s1) + s2) + s3 is the four-wave kernel's own order
// (each wave holds one slab), and a large weight (2.4 M outputs) needs 9,216 workgroups instead of 36,864 -- that many
// 64-output workgroups were bound by the workgroup launch rate, not by the 4 slabs' 38 MB.
__global__ __launch_bounds__(256) void slab_reduce_few_kernel(const float* __restrict__ slabs, float* __restrict__ gw,
                                                              int Z, int Mp, int Jp, int Co, int C, int T,
                                                              const float* __restrict__ bslab, float* __restrict__ gb) {
    const long long total = (long long)Co * C * T;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) {
        // bias gradient: the weight-gradient GEMM's row sums per split (bslab[z][Mp]), same fixed order
        const long long o = i - total;
        if (bslab && o < Co) {
            float v[4];
#pragma unroll
            for (int z = 0; z < 4; ++z) v[z] = z < Z ? 0.0f + bslab[(size_t)z * Mp + o] : 0.0f;
            gb[o] = ((v[0] + v[1]) + v[2]) + v[3];
        }
        return;
    }
    const int K = T * C;
    const int j = (int)(i % K), o = (int)(i / K);
    const size_t off = (size_t)o * Jp + j, zs = (size_t)Mp * Jp;
    float v[4];
#pragma unroll
    for (int z = 0; z < 4; ++z) v[z] = z < Z ? 0.0f + slabs[(size_t)z * zs + off] : 0.0f;   // (0 + x: the wave's start)
    const int tap = j / C, c = j - tap * C;
    gw[((size_t)o * C + c) * T + tap] = ((v[0] + v[1]) + v[2]) + v[3];
}

// gw[o][c][tap] = sum_z slabs[z][o][tap*C + c].  Workgroup = 64 consecutive outputs x 4 waves; wave w sums
// slabs w, w+4, w+8, ... (coalesced 256-B rows), the four partial sums are added in wave order through LDS:
// a fixed summation order (bit-reproducible) with 4x the parallelism of one thread per output.
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ gw,
                                                          int Z, int Mp, int Jp, int Co, int C, int T,
                                                          const float* __restrict__ bslab, float* __restrict__ gb) {
    __shared__ float part[4][64];
    const long long total = (long long)Co * C * T;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * 64 + lane;
    // outputs [total, total + Co): the bias gradient from the GEMM's per-split row sums (bslab[z][Mp]), summed like a
    // weight element -- wave w takes splits w, w + 4, ..., the four partial sums are added in wave order
    const bool is_bias = bslab != nullptr && i >= total && i < total + Co;
    float s = 0.0f;
    if (i < total || is_bias) {
        // enumerate in slab order (j = tap*C + c contiguous): coalesced reads, strided (small) writes
        const int K = T * C;
        const int j = (int)(i % K), o = (int)(i / K);
        if (is_bias) slabs = bslab;
        const size_t off = is_bias ? (size_t)(i - total) : (size_t)o * Jp + j;
        // same order of additions as a plain loop; the loads of eight slabs are in flight together (the loop is
        // latency-bound: up to ~60 slabs, 14 dependent round trips per wave otherwise)
        const size_t zs = is_bias ? (size_t)Mp : (size_t)Mp * Jp;
        for (int z = w; z < Z; z += 32) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = z + 4 * u < Z ? slabs[(size_t)(z + 4 * u) * zs + off] : 0.0f;
#pragma unroll
            for (int u = 0; u < 8; ++u) if (z + 4 * u < Z) s += v[u];
        }
    }
    part[w][lane] = s;
    __syncthreads();
    if (w == 0 && is_bias) gb[i - total] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    if (w == 0 && i < total) {
        const int K = T * C;
        const int j = (int)(i % K), o = (int)(i / K);
        const int tap = j / C, c = j - tap * C;
        gw[((size_t)o * C + c) * T + tap] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    }
}

// out[c] = sum over (b, hw) of x[b][c][hw]: the bias gradient of the paths that have no weight-gradient GEMM to take it
// from (the LDS-tile kernels of the 3- / 16-channel layers, deformable_group > 1).  Everything else gets it from
// igemm_wgrad_*_kernel's own staging registers (bslab) and slab_reduce_*.
__global__ __launch_bounds__(256) void channel_sum_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                          int B, int C, long long HW) {
    __shared__ float red[16];
    const int c = blockIdx.x;
    float s = 0.0f;
    for (int b = 0; b < B; ++b) {
        const float* p = x + ((size_t)b * C + c) * HW;
        for (long long i = threadIdx.x; i < HW; i += 256) s += p[i];
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[c] = s;
}

// ---------------------------------------------------------------------------
// Pack cache.  The packed weight image only changes when the weights do (once per optimizer step), yet every
// convolution call used to rebuild it: 282 tiny launches per training step.  The host layer owns the memory
// (cnuda_pack_cache_attach: one caller-allocated arena, nothing is allocated in here) and the notion of weight
// identity: before a call it announces a STAMP = (token of the module that owns the weights, version of the
// weights) with cnuda_pack_stamp.  A slot is reused iff the same token asked for the same image of the same source
// buffer before and the version is unchanged; token 0 (the default, and every caller that says nothing) bypasses
// the cache.  One stamp covers every pack of the entry point that follows it (and of the calls nested in it).
// The arena and its slots are PROCESS-global (one process drives one GPU: DESIGN.md section 7); a module that asks
// for an image of a new source buffer takes over its own old slot.
// ---------------------------------------------------------------------------
struct PackKey {
    uint64_t token;
    const void* src;
    int mode, Co, C, T, Kp, Mp, extra;
    bool operator==(const PackKey& o) const {
        return token == o.token && src == o.src && mode == o.mode && Co == o.Co && C == o.C && T == o.T && Kp == o.Kp &&
               Mp == o.Mp && extra == o.extra;
    }
};
struct PackKeyHash {
    size_t operator()(const PackKey& k) const {
        uint64_t h = k.token * 0x9E3779B97F4A7C15ull ^ (uint64_t)(uintptr_t)k.src;
        const int v[7] = {k.mode, k.Co, k.C, k.T, k.Kp, k.Mp, k.extra};
        for (int x : v) h = (h ^ (uint64_t)(unsigned)x) * 0xBF58476D1CE4E5B9ull;
        return (size_t)(h ^ (h >> 31));
    }
};
struct PackSlot {
    size_t offset, bytes;
    uint64_t version;
    int cpad;            // PACK_DGRAD: channels per tap on the K axis
    int ntaps, taps[9];  // mode 2 (tap subset)
};
std::mutex g_pack_mutex;                      // forward runs on the caller's thread, backward on autograd's
std::unordered_map<PackKey, PackSlot, PackKeyHash> g_pack_slots;
char* g_pack_arena = nullptr;
size_t g_pack_arena_bytes = 0, g_pack_arena_used = 0;
uint64_t g_pack_generation = 0;               // bumped when a slot is added (the refresh table is rebuilt then)
std::atomic<unsigned long long> g_pack_fills{0};   // cached images (re)written on a convolution's own call
// Eviction.  The arena is a bump allocator and a module that is gone (a model deleted, a plugin rebuilt: bench.py's
// other_configs legs, a test session) never returns its slots, so a long-lived process would fill the arena and then
// silently stop caching.  When a slot does not fit, the request is served from the caller's workspace and a RESET is
// scheduled; it happens at the next cnuda_pack_stamp of a cached call -- never in the middle of an entry point, whose
// earlier packs may still be in flight in slots a reset would hand out again -- and forgets every slot: the live
// modules re-pack once, on the launch stream, in stream order behind everything that still reads the old images.
// A working set LARGER than the arena (teacher + student, a small CNUDA_PACK_CACHE_MB) would fill it again within one
// step of every reset and re-pack everything every step: a reset is therefore only honoured when at least
// g_pack_reset_min_stamps stamped calls have gone by since the previous one, and that distance doubles with every reset
// (1,024 stamps ~ 7 DLA-34 steps at first) -- in between, the slots that fit stay cached and only the overflow is
// served from the workspace, which is what the cache did before it had a reset.
// Threading: the stamp / slot state is per process; the library expects ONE thread at a time inside its convolution
// entry points (torch runs backward() on its device thread while the caller's thread blocks, so a training loop
// satisfies this by construction).  Two threads driving convolutions concurrently must not share a pack arena.
std::atomic<bool> g_pack_reset_wanted{false};
std::atomic<unsigned long long> g_pack_resets{0};
unsigned long long g_pack_stamps_since_reset = ~0ull >> 1, g_pack_reset_min_stamps = 0;
thread_local uint64_t g_pack_token = 0, g_pack_version = 0;

// -> cached slot to use (fill == true: pack into it first), or nullptr: use the workspace
constexpr size_t kPackSlack = 4096;
float* pack_slot(const PackKey& key, size_t bytes, bool& fill, int cpad = 0, const TapList* taps = nullptr) {
    fill = true;
    if (key.token == 0 || !g_pack_arena) return nullptr;
    std::lock_guard<std::mutex> lock(g_pack_mutex);
    auto it = g_pack_slots.find(key);
    if (it == g_pack_slots.end()) {
        // the same module asking for the same image of a NEW source buffer (a re-fold of BatchNorm allocates fresh
        // folded weights every time): its old slot is dead -- take it over instead of growing until the arena is full
        for (auto old = g_pack_slots.begin(); old != g_pack_slots.end(); ++old) {
            const PackKey& k = old->first;
            if (k.token == key.token && k.src != key.src && k.mode == key.mode && k.Co == key.Co && k.C == key.C &&
                k.T == key.T && k.Kp == key.Kp && k.Mp == key.Mp && k.extra == key.extra && old->second.bytes >= bytes) {
                PackSlot moved = old->second;
                moved.version = ~0ull;
                g_pack_slots.erase(old);
                it = g_pack_slots.emplace(key, moved).first;
                ++g_pack_generation;
                break;
            }
        }
    }
    if (it == g_pack_slots.end()) {
        // (+ kPackSlack: the 32-row split-operand kernel of matrix mode 1 read up to 1 KB past the end of its image (a clamp
        // in igemm.cuh ig_load_a_x3 that pointed outside the tile, fixed in round 6) -- harmless inside the workspace or the
        // arena, an abort when the slot was the arena's last bytes, i.e. once a session's later models had filled the 768 MB.
        // The slack stays: no kernel's read-ahead may depend on what lies behind the arena)
        const size_t need = (bytes + 255) / 256 * 256 + kPackSlack;
        if (g_pack_arena_used + need > g_pack_arena_bytes) {                      // arena full: this request goes to the
            g_pack_reset_wanted = need <= g_pack_arena_bytes;                     // workspace, the cache starts over at
            return nullptr;                                                       // the next stamped call
        }
        it = g_pack_slots.emplace(key, PackSlot{g_pack_arena_used, bytes, ~0ull, 0, 0, {0}}).first;
        g_pack_arena_used += need;
        ++g_pack_generation;
    }
    if (it->second.bytes < bytes) return nullptr;
    it->second.cpad = cpad;
    if (taps) { it->second.ntaps = taps->n; for (int i = 0; i < 9; ++i) it->second.taps[i] = taps->tap[i]; }
    fill = it->second.version != g_pack_version;
    if (fill) ++g_pack_fills;
    it->second.version = g_pack_version;
    return reinterpret_cast<float*>(g_pack_arena + it->second.offset);
}

}  // namespace

PackStampSuspend::PackStampSuspend() : token(g_pack_token), version(g_pack_version) { g_pack_token = 0; g_pack_version = 0; }
PackStampSuspend::~PackStampSuspend() { g_pack_token = token; g_pack_version = version; }

const float* launch_pack(const float* W, float* dst, size_t room, int Co, int C, int T, PackMode mode, int Kp, int Mp,
                         int Cpad, hipStream_t st) {
    bool fill = true;
    const PackKey key{g_pack_token, W, (int)mode, Co, C, T, Kp, Mp, Cpad};
    if (float* slot = pack_slot(key, room, fill, Cpad)) dst = slot;
    if (fill) {
        const long long total = (long long)Kp * Mp;
        CNUDA_LAUNCH(pack_kernel, dim3(stream_grid(total, 256)), dim3(256), 0, st, W, dst, Co, C, T, (int)mode, Kp,
                           Mp, Cpad);
    }
    return dst;
}

const float* launch_pack_taps(const float* W, float* dst, size_t room, int Co, int C, int T, const int* taps, int ntaps,
                              int Kp, int Mp, hipStream_t st) {
    TapList tl;
    tl.n = ntaps;
    int sig = ntaps;
    for (int i = 0; i < 9; ++i) { tl.tap[i] = i < ntaps ? taps[i] : 0; sig = sig * 31 + tl.tap[i]; }
    bool fill = true;
    const PackKey key{g_pack_token, W, 2, Co, C, T, Kp, Mp, sig};
    if (float* slot = pack_slot(key, room, fill, 0, &tl)) dst = slot;
    if (fill) {
        const long long total = (long long)Kp * Mp;
        CNUDA_LAUNCH(pack_taps_kernel, dim3(stream_grid(total, 256)), dim3(256), 0, st, W, dst, Co, C, T, tl, Kp, Mp);
    }
    return dst;
}

void launch_slab_reduce(const float* slabs, float* gw, int Z, int Mp, int Jp, int Co, int C, int T, hipStream_t st,
                        const float* bslab, float* gb) {
    const long long total = (long long)Co * C * T, outs = total + (bslab ? Co : 0);
    if (Z <= 4 && total >= (1 << 18))       // (the large weights are the ones with few slabs)
        CNUDA_LAUNCH(slab_reduce_few_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, st, slabs, gw, Z,
                           Mp, Jp, Co, C, T, bslab, gb);
    else
        CNUDA_LAUNCH(slab_reduce_kernel, dim3((unsigned)((outs + 63) / 64)), dim3(256), 0, st, slabs, gw, Z, Mp,
                           Jp, Co, C, T, bslab, gb);
}

void launch_channel_sum(const float* x, float* out, int B, int C, long long HW, hipStream_t st) {
    CNUDA_LAUNCH(channel_sum_kernel, dim3(C), dim3(256), 0, st, x, out, B, C, HW);
}

}  // namespace cnuda

extern "C" int cnuda_pack_cache_attach(void* arena, size_t bytes) {
    std::lock_guard<std::mutex> lock(cnuda::g_pack_mutex);
    cnuda::g_pack_slots.clear();
    cnuda::g_pack_arena = reinterpret_cast<char*>(((uintptr_t)arena + 255) & ~(uintptr_t)255);
    cnuda::g_pack_arena_bytes = arena ? bytes - (size_t)(cnuda::g_pack_arena - (char*)arena) : 0;
    cnuda::g_pack_arena_used = 0;
    cnuda::g_pack_reset_wanted = false;
    cnuda::g_pack_stamps_since_reset = ~0ull >> 1;       // a fresh arena: its first overflow may reset at once
    cnuda::g_pack_reset_min_stamps = 0;
    ++cnuda::g_pack_generation;
    if (!arena) cnuda::g_pack_arena = nullptr;
    return 0;
}
// ---------------------------------------------------------------------------
// Refresh after an optimizer step: every cached image whose source lies in the optimizer's parameter arena and
// that was current in the epoch that just ended is rebuilt by ONE launch (a table of pack jobs, one workgroup per
// 2048 elements) and stamped with the new epoch -- instead of ~150 five-microsecond launches spread over the next
// step, each of which leaves the chip idle.
// ---------------------------------------------------------------------------
namespace cnuda {
namespace {
struct PackJob {
    const float* src;
    float* dst;
    int mode, Co, C, T, Kp, Mp, cpad, ntaps;
    int taps[9];
    unsigned block0;          // first workgroup of this job
};
constexpr int PJ_PER_BLOCK = 2048;
__global__ __launch_bounds__(256) void pack_multi_kernel(const PackJob* __restrict__ jobs, int njobs) {
    // the job whose block range holds blockIdx.x (jobs are sorted by block0)
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].block0 <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const PackJob j = jobs[lo];
    const long long total = (long long)j.Kp * j.Mp;
    const long long base = (long long)(blockIdx.x - j.block0) * PJ_PER_BLOCK;
    for (int t = threadIdx.x; t < PJ_PER_BLOCK; t += 256) {
        const long long i = base + t;
        if (i >= total) break;
        const int k = (int)(i / j.Mp), m = (int)(i % j.Mp);
        float v = 0.0f;
        if (j.mode == PACK_FWD) {
            if (k < j.T * j.C && m < j.Co) v = j.src[((size_t)m * j.C + k % j.C) * j.T + k / j.C];
        } else if (j.mode == PACK_HALO_FWD) {
            if (k < j.T * j.C && m < j.Co) {
                const int g = k / (16 * j.T), r = k - g * 16 * j.T;
                v = j.src[((size_t)m * j.C + 16 * g + (r & 15)) * j.T + (r >> 4)];
            }
        } else if (j.mode == PACK_HALO_DGRAD) {
            if (k < j.T * j.Co && m < j.C) {
                const int g = k / (16 * j.T), r = k - g * 16 * j.T;
                v = j.src[((size_t)(16 * g + (r & 15)) * j.C + m) * j.T + (j.T - 1 - (r >> 4))];
            }
        } else if (j.mode == PACK_DGRAD) {
            if (k < j.T * j.cpad && m < j.C) {
                const int tap = k / j.cpad, o = k % j.cpad;
                if (o < j.Co) v = j.src[((size_t)o * j.C + m) * j.T + tap];
            }
        } else {
            if (k < j.ntaps * j.Co && m < j.C) {
                const int ti = k / j.Co, o = k - ti * j.Co;
                v = j.src[((size_t)o * j.C + m) * j.T + j.taps[ti]];
            }
        }
        j.dst[i] = v;
    }
}
std::vector<PackJob> g_refresh_jobs;
unsigned g_refresh_blocks = 0;
const void* g_refresh_table = nullptr;        // the device buffer the current job list was uploaded to
}  // namespace
}  // namespace cnuda

extern "C" int cnuda_pack_refresh_ranges(const void* const* params, const size_t* params_bytes, int ranges,
                                         unsigned long long old_epoch, unsigned long long new_epoch, void* table,
                                         size_t table_bytes, cnuda_stream_t stream) {
    using namespace cnuda;
    CNUDA_REQUIRE(ranges >= 0 && (ranges == 0 || (params && params_bytes)), "cnuda_pack_refresh_ranges: null ranges");
    std::lock_guard<std::mutex> lock(g_pack_mutex);
    if (!g_pack_arena || g_pack_slots.empty() || ranges == 0) return 0;
    auto rewritten = [&](const char* src) {
        for (int r = 0; r < ranges; ++r) {
            const char* lo = static_cast<const char*>(params[r]);
            if (src >= lo && src < lo + params_bytes[r]) return true;
        }
        return false;
    };
    hipStream_t st = (hipStream_t)stream;
    // jobs: slots whose source lies inside a rewritten buffer and whose image was current in the epoch that just ended
    // (anything else refills lazily on its next use)
    std::vector<PackSlot*> live;
    std::vector<PackJob> jobs;
    unsigned blocks = 0;
    for (auto& kv : g_pack_slots) {
        const char* src = static_cast<const char*>(kv.first.src);
        if (kv.first.token == 0 || !rewritten(src)) continue;
        if ((kv.second.version >> 32) != (old_epoch & 0xffffffffull)) continue;
        live.push_back(&kv.second);
        PackJob j;
        memset(&j, 0, sizeof(j));
        j.src = static_cast<const float*>(kv.first.src);
        j.dst = reinterpret_cast<float*>(g_pack_arena + kv.second.offset);
        j.mode = kv.first.mode; j.Co = kv.first.Co; j.C = kv.first.C; j.T = kv.first.T;
        j.Kp = kv.first.Kp; j.Mp = kv.first.Mp; j.cpad = kv.second.cpad; j.ntaps = kv.second.ntaps;
        for (int i = 0; i < 9; ++i) j.taps[i] = kv.second.taps[i];
        j.block0 = blocks;
        jobs.push_back(j);
        blocks += (unsigned)(((long long)kv.first.Kp * kv.first.Mp + PJ_PER_BLOCK - 1) / PJ_PER_BLOCK);
    }
    if (live.empty()) return 0;
    // the table only changes when the set of live slots does: upload it then, reuse the device copy otherwise
    // (a table that does not fit, or none: nothing is refreshed here -- the parameters are already updated, so this
    // must not fail the optimizer step; the slots keep their old epoch and refill lazily on their next use)
    if (!table || jobs.size() * sizeof(PackJob) > table_bytes) return 0;
    if (table != g_refresh_table || jobs.size() != g_refresh_jobs.size() ||
        memcmp(jobs.data(), g_refresh_jobs.data(), jobs.size() * sizeof(PackJob)) != 0) {
        g_refresh_table = table;      // (a caller that re-allocated its table -- another device -- gets a fresh upload)
        g_refresh_jobs = jobs;        // (the copy below reads this vector: it must outlive the call)
        if (hipMemcpyAsync(table, g_refresh_jobs.data(), g_refresh_jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice,
                           st) != hipSuccess)
            return check_launch("cnuda_pack_refresh(table)");
        g_refresh_blocks = blocks;
    }
    CNUDA_LAUNCH(pack_multi_kernel, dim3(g_refresh_blocks), dim3(256), 0, st, static_cast<const PackJob*>(table),
                       (int)g_refresh_jobs.size());
    for (PackSlot* sl : live) sl->version = ((new_epoch & 0xffffffffull) << 32) | (sl->version & 0xffffffffull);
    return check_launch("cnuda_pack_refresh");
}

extern "C" int cnuda_pack_refresh(const void* params, size_t params_bytes, unsigned long long old_epoch,
                                  unsigned long long new_epoch, void* table, size_t table_bytes,
                                  cnuda_stream_t stream) {
    return cnuda_pack_refresh_ranges(&params, &params_bytes, 1, old_epoch, new_epoch, table, table_bytes, stream);
}

extern "C" int cnuda_pack_stamp(unsigned long long token, unsigned long long version) {
    using namespace cnuda;
    if (token != 0) ++g_pack_stamps_since_reset;
    if (token != 0 && g_pack_reset_wanted) {
        std::lock_guard<std::mutex> lock(g_pack_mutex);
        if (g_pack_reset_wanted && g_pack_stamps_since_reset < g_pack_reset_min_stamps) {
            g_pack_reset_wanted = false;     // too soon after the last one: the live set does not fit, keep what does
        } else if (g_pack_reset_wanted) {
            g_pack_stamps_since_reset = 0;
            g_pack_reset_min_stamps = g_pack_reset_min_stamps ? (g_pack_reset_min_stamps < (1ull << 20) ? 2 * g_pack_reset_min_stamps
                                                                                                      : g_pack_reset_min_stamps)
                                                              : 1024;
            g_pack_slots.clear();
            g_pack_arena_used = 0;
            ++g_pack_generation;
            g_refresh_table = nullptr;       // (the next refresh uploads its job list afresh)
            g_pack_reset_wanted = false;
            ++g_pack_resets;
        }
    }
    g_pack_token = token;
    g_pack_version = version;
    return 0;
}
extern "C" unsigned long long cnuda_pack_cache_resets(void) { return cnuda::g_pack_resets.load(); }
extern "C" size_t cnuda_pack_cache_used(void) { return cnuda::g_pack_arena_used; }
extern "C" unsigned long long cnuda_pack_cache_fills(void) { return cnuda::g_pack_fills.load(); }
