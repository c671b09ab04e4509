// A streaming tick with its session state on the device (include/pwv_hip.h, "A streaming TICK" and "A RAGGED streaming tick"): the two
// small kernels that stand at the two ends of a captured push.  The begin kernel turns the session table into the launch tables of the
// tick (slot table, noise streams, cu_rows / cu_frames, the chunk's frames with every session's kept frame in front); the commit kernel,
// the tick's last node, advances the sessions iff the tick's launches left both sticky words clean.  A UNIFORM tick is a ragged tick
// whose frame counts are all equal: both bodies are written once over a COUNTS policy that says where entry i's frames begin --
// UniformCounts in closed form, RaggedCounts from the device table, clamped so that the packed layout is well formed whatever the table
// holds.  A ragged tick may START utterances (include/pwv_hip.h, "STARTS"): both bodies have a STARTS form, instantiated as kernels of
// their own, in which an entry whose flag is set reads the zero block and its first frame from the caller's table and is committed with
// its counter set and its seed written.  Plain C++, every address from the arguments, vector stores only.
#include <cstddef>

#include "pwv_common.h"

namespace pwv {

constexpr int RAGGED_MAX_N = 1024;

// Both ticks.  frames: of every entry (uniform) / the fewest of an entry (ragged); step: samples per entry (uniform: T) / per frame
// (ragged: hop); in_frames: the frames of all N entries (uniform: N * frames).  The chunk is [in_frames + N][n_mels] -- the uniform
// [N][frames + 1][n_mels] is that with cu(i) = i * frames.
struct TickParams {
    long long* sess;
    float* kept;
    const int* entries;
    const float* mel;
    int n_slots, N, in_frames, n_mels, frames, step;
    int* slot_tab;
    unsigned long long* streams;
    int* cu_rows;
    int* cu_frames;
    float* chunk;
    const int* words;
    long long* counters;
    // the STARTS form alone reads these (a ragged tick with starts): {flag, seed bits} and the first frame per entry, the block of zeros
    const long long* starts;
    const float* first;
    int zero_block;
};

// A counts policy: prepare() once per workgroup, by all its threads (it ends on a barrier), then cu(i) -- the frames in front of entry
// i, 0 .. N --, rows(i) -- the samples --, slot(i) / live(i) -- a slot outside the table is a filler of slot 0, so no address leaves
// the arrays -- and entry_of(row), the entry chunk row `row` belongs to: the last i with cu(i) + i <= row.

// every entry p.frames frames: closed form, the entries read at stride 2 where they are needed, nothing in LDS, any N
struct UniformCounts {
    const TickParams& p;
    __device__ void prepare() { __syncthreads(); }          // (nothing of its own: the barrier publishes the commit's decision)
    __device__ int cu(int i) const { return i * p.frames; }
    __device__ int rows(int i) const { return i * p.step; }
    __device__ int slot(int i) const {
        const int s = p.entries[2 * i];
        return (unsigned)s < (unsigned)p.n_slots ? s : 0;
    }
    __device__ int live(int i) const { return (unsigned)p.entries[2 * i] < (unsigned)p.n_slots ? p.entries[2 * i + 1] : 0; }
    __device__ int entry_of(int row) const { return row / (p.frames + 1); }
};

// The frame counts as the device reads them from entries {slot, live, frames, 0}, by every workgroup for itself: cu[0 .. N] (prefix sums
// of the clamped counts, cu[N] = in_frames), slot[0 .. N-1] and, for the commit (LIVE), live[0 .. N-1] in LDS.  Whatever `entries`
// holds, cu rises by at least p.frames per entry and ends at in_frames: no address derived from it leaves the arrays.
template <bool LIVE>
struct RaggedCounts {
    const TickParams& p;
    int *cu_, *slot_, *live_;
    __device__ void prepare() {
        __shared__ int cu[RAGGED_MAX_N + 1], slot[RAGGED_MAX_N];
        cu_ = cu, slot_ = slot, live_ = nullptr;
        if constexpr (LIVE) {
            __shared__ int live[RAGGED_MAX_N];
            live_ = live;
        }
        for (int i = threadIdx.x; i < p.N; i += blockDim.x) {
            const int s = p.entries[4 * i];
            const bool ok = (unsigned)s < (unsigned)p.n_slots;
            slot[i] = ok ? s : 0;
            if constexpr (LIVE) live_[i] = ok ? p.entries[4 * i + 1] : 0;
            cu[i + 1] = p.entries[4 * i + 2];          // (the wanted count, replaced by the prefix sum below)
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int at = 0;
            cu[0] = 0;
            for (int i = 0; i < p.N - 1; ++i) {
                const int most = p.in_frames - at - (p.N - 1 - i) * p.frames;      // >= p.frames: in_frames >= N * frames
                const int want = cu[i + 1];
                at += want < p.frames ? p.frames : (want > most ? most : want);
                cu[i + 1] = at;
            }
            cu[p.N] = p.in_frames;
        }
        __syncthreads();
    }
    __device__ int cu(int i) const { return cu_[i]; }
    __device__ int rows(int i) const { return p.step * cu_[i]; }
    __device__ int slot(int i) const { return slot_[i]; }
    __device__ int live(int i) const { return live_[i]; }
    __device__ int entry_of(int row) const {          // (cu[i] + i rises strictly; cu[0] + 0 = 0 <= row)
        int lo = 0, hi = p.N - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (cu_[mid] + mid <= row) lo = mid; else hi = mid - 1;
        }
        return lo;
    }
};

// STARTS form: does entry i begin a new utterance?  Its flag is set and it is no filler (live, slot inside the table).  The flag is all
// that is read of the starts table to decide an address.
__device__ inline bool tick_starting(const TickParams& p, int i) {
    return p.starts[2 * i] != 0 && p.entries[4 * i + 1] != 0 && (unsigned)p.entries[4 * i] < (unsigned)p.n_slots;
}

// one thread per float of the chunk; workgroup 0 also writes the tables
template <class Counts, bool STARTS = false>
__device__ inline void tick_begin(const TickParams& p) {
    Counts n{p};
    n.prepare();
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i <= p.N; i += blockDim.x) {
            if (p.cu_rows) p.cu_rows[i] = n.rows(i);
            if (p.cu_frames) p.cu_frames[i] = n.cu(i) + i;
            if (i == p.N) break;
            const int s = n.slot(i);
            const int g = (int)(p.sess[4 * (long long)s] & 1);
            bool starting = false;
            if constexpr (STARTS) starting = tick_starting(p, i);
            p.slot_tab[2 * i] = starting ? p.zero_block : 2 * s + g;
            p.slot_tab[2 * i + 1] = 2 * s + 1 - g;
            if (p.streams) {
                p.streams[2 * i] = (unsigned long long)(starting ? p.starts[2 * i + 1] : p.sess[4 * (long long)s + 2]);
                p.streams[2 * i + 1] = starting ? 0ull : (unsigned long long)p.sess[4 * (long long)s + 1];
            }
        }
    }
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)(p.in_frames + p.N) * p.n_mels) return;
    const int row = (int)(idx / p.n_mels), c = (int)(idx % p.n_mels);
    const int i = n.entry_of(row);
    const int f = row - (n.cu(i) + i);          // 0 .. f_i: row < cu(i + 1) + i + 1
    if constexpr (STARTS) {
        if (f == 0 && tick_starting(p, i)) {          // (the utterance's first frame stands where the kept frame would)
            p.chunk[idx] = p.first[(long long)i * p.n_mels + c];
            return;
        }
    }
    p.chunk[idx] = f == 0 ? p.kept[(long long)n.slot(i) * p.n_mels + c] : p.mel[(long long)(n.cu(i) + f - 1) * p.n_mels + c];
}

// ONE workgroup: the words are read once, so all entries of a tick see one decision
template <class Counts, bool STARTS = false>
__device__ inline void tick_commit(const TickParams& p) {
    __shared__ int clean;
    if (threadIdx.x == 0) {
        const int gave_up = __hip_atomic_load(p.words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const int range = __hip_atomic_load(p.words + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        clean = (gave_up == 0 && range == 0) ? 1 : 0;
        p.counters[clean ? 0 : 1] += 1;
    }
    Counts n{p};
    n.prepare();          // (its barrier publishes `clean` too)
    if (!clean) return;
    for (int i = threadIdx.x; i < p.N; i += blockDim.x) {
        if (n.live(i)) {
            const int s = n.slot(i);
            p.sess[4 * (long long)s] ^= 1;
            if constexpr (STARTS) {
                if (p.starts[2 * i] != 0) {          // (live: a start, with the counter set and the seed the utterance draws from)
                    p.sess[4 * (long long)s + 1] = n.rows(i + 1) - n.rows(i);
                    p.sess[4 * (long long)s + 2] = p.starts[2 * i + 1];
                    continue;
                }
            }
            p.sess[4 * (long long)s + 1] += n.rows(i + 1) - n.rows(i);
        }
    }
    const int total = p.N * p.n_mels;
    for (int k = threadIdx.x; k < total; k += blockDim.x) {
        const int i = k / p.n_mels, c = k % p.n_mels;
        if (n.live(i)) p.kept[(long long)n.slot(i) * p.n_mels + c] = p.mel[(long long)(n.cu(i + 1) - 1) * p.n_mels + c];
    }
}

__global__ void stream_tick_begin_kernel(TickParams p) { tick_begin<UniformCounts>(p); }
__global__ void stream_tick_commit_kernel(TickParams p) { tick_commit<UniformCounts>(p); }
__global__ void stream_tick_ragged_begin_kernel(TickParams p) { tick_begin<RaggedCounts<false>>(p); }
__global__ void stream_tick_ragged_commit_kernel(TickParams p) { tick_commit<RaggedCounts<true>>(p); }
__global__ void stream_tick_starts_begin_kernel(TickParams p) { tick_begin<RaggedCounts<false>, true>(p); }
__global__ void stream_tick_starts_commit_kernel(TickParams p) { tick_commit<RaggedCounts<true>, true>(p); }

// ---- the entry points: everything is decided before a device is needed ---------------------------------------------------------------

// what the four entry points check alike, on what their adapter has filled in; begin: the call is a tick's first node, else its last
static int tick_check(const TickParams& p, const char* who, bool begin) {
    PWV_CHECK_ARG(p.sess, "%s: sess is NULL", who);
    PWV_CHECK_ARG(p.kept, "%s: kept is NULL", who);
    PWV_CHECK_ARG(p.entries, "%s: entries is NULL", who);
    PWV_CHECK_ARG(p.mel, "%s: mel is NULL", who);
    PWV_CHECK_ARG(p.n_slots >= 1, "%s: n_slots must be >= 1, got %d", who, p.n_slots);
    PWV_CHECK_ARG(p.n_mels >= 1, "%s: n_mels must be >= 1, got %d", who, p.n_mels);
    if (begin) {
        PWV_CHECK_ARG(p.slot_tab, "%s: slot_tab is NULL", who);
        PWV_CHECK_ARG(p.chunk, "%s: chunk is NULL", who);
    } else {
        PWV_CHECK_ARG(p.words, "%s: words is NULL", who);
        PWV_CHECK_ARG(p.counters, "%s: counters is NULL", who);
    }
    return PWV_OK;
}

// `need`: the bytes of `type` the call cannot do without (the whole struct, or what stands in front of its optional trailing fields)
#define PWV_TICK_STRUCT(a, type, need)                                                                                           \
    PWV_CHECK_ARG(a, "%s: args is NULL", who);                                                                                   \
    PWV_CHECK_ARG(a->struct_size >= (need), "%s: struct_size %zu is short of " #type " (%zu bytes)", who, a->struct_size,       \
                  (size_t)(need))

// an optional trailing field: what the caller's struct holds of it, else zero
#define PWV_TICK_OPTIONAL(a, type, field) \
    (a->struct_size >= offsetof(type, field) + sizeof(a->field) ? a->field : decltype(a->field){})

// the uniform tick: frames and T per entry, streams and cu_rows together or not at all, no cu_frames, any N
static int tick_params(const pwv_stream_tick_args* a, const char* who, bool begin, TickParams* p) {
    PWV_TICK_STRUCT(a, pwv_stream_tick_args, sizeof(pwv_stream_tick_args));
    *p = TickParams{(long long*)a->sess, a->kept, a->entries, a->mel, a->n_slots, a->N, 0, a->n_mels, a->frames, a->T, a->slot_tab,
                    (unsigned long long*)a->streams, a->cu_rows, nullptr, a->chunk, a->words, (long long*)a->counters, nullptr, nullptr, 0};
    const int rc = tick_check(*p, who, begin);
    if (rc != PWV_OK) return rc;
    PWV_CHECK_ARG(a->N >= 1, "%s: N must be >= 1, got %d", who, (int)a->N);
    PWV_CHECK_ARG(a->frames >= 1, "%s: frames must be >= 1, got %d", who, (int)a->frames);
    PWV_CHECK_ARG(a->T >= 1, "%s: T must be >= 1, got %d", who, (int)a->T);
    PWV_CHECK_ARG((long long)a->N * a->T < (1ll << 31) && (long long)a->N * ((long long)a->frames + 1) * a->n_mels < (1ll << 31),
                  "%s: N * T and N * (frames + 1) * n_mels must stay below 2^31", who);
    PWV_CHECK_ARG(!begin || (a->streams == nullptr) == (a->cu_rows == nullptr), "%s: streams and cu_rows go together (both or neither)", who);
    p->in_frames = a->N * a->frames;
    return PWV_OK;
}

// the ragged tick: the counts in LDS (N <= RAGGED_MAX_N), cu_rows and cu_frames the launches' layout with or without streams; starts,
// first and zero_block are optional trailing fields (a struct that ends in front of one reads it as zero)
static int tick_params(const pwv_stream_tick_ragged_args* a, const char* who, bool begin, TickParams* p) {
    PWV_TICK_STRUCT(a, pwv_stream_tick_ragged_args, offsetof(pwv_stream_tick_ragged_args, starts));
    *p = TickParams{(long long*)a->sess, a->kept, a->entries, a->mel, a->n_slots, a->N, a->in_frames, a->n_mels, a->min_frames, a->hop,
                    a->slot_tab, (unsigned long long*)a->streams, a->cu_rows, a->cu_frames, a->chunk, a->words, (long long*)a->counters,
                    (const long long*)PWV_TICK_OPTIONAL(a, pwv_stream_tick_ragged_args, starts),
                    PWV_TICK_OPTIONAL(a, pwv_stream_tick_ragged_args, first), PWV_TICK_OPTIONAL(a, pwv_stream_tick_ragged_args, zero_block)};
    const int rc = tick_check(*p, who, begin);
    if (rc != PWV_OK) return rc;
    PWV_CHECK_ARG(a->N >= 1 && a->N <= RAGGED_MAX_N, "%s: N must be 1 .. %d, got %d", who, RAGGED_MAX_N, (int)a->N);
    PWV_CHECK_ARG(a->hop >= 1, "%s: hop must be >= 1, got %d", who, (int)a->hop);
    PWV_CHECK_ARG(a->min_frames >= 1, "%s: min_frames must be >= 1, got %d", who, (int)a->min_frames);
    PWV_CHECK_ARG((long long)a->in_frames >= (long long)a->N * a->min_frames, "%s: in_frames must be >= N * min_frames = %lld, got %d", who,
                  (long long)a->N * a->min_frames, (int)a->in_frames);
    PWV_CHECK_ARG((long long)a->in_frames * a->hop < (1ll << 31) && ((long long)a->in_frames + a->N) * a->n_mels < (1ll << 31),
                  "%s: in_frames * hop and (in_frames + N) * n_mels must stay below 2^31", who);
    PWV_CHECK_ARG(!begin || a->cu_rows, "%s: cu_rows is NULL (required with or without streams: the launches' layout)", who);
    PWV_CHECK_ARG(!begin || a->cu_frames, "%s: cu_frames is NULL", who);
    if (p->starts) {
        PWV_CHECK_ARG(p->first, "%s: first is NULL (required with starts: the first frame of a starting entry)", who);
        PWV_CHECK_ARG((long long)p->zero_block >= 2ll * a->n_slots, "%s: zero_block must be >= 2 * n_slots = %lld (no session's block), got %d",
                      who, 2ll * a->n_slots, p->zero_block);
    }
    return PWV_OK;
}

// check, then one launch: the begin kernel with a thread per float of the chunk, the commit kernel as ONE workgroup; `with_starts` is
// the kernel of a tick that brings a starts table (the ragged tick alone has one)
template <class Args>
static int tick_launch(const Args* a, const char* who, bool begin, void (*kernel)(TickParams), pwv_stream_t stream,
                       void (*with_starts)(TickParams) = nullptr) {
    TickParams p{};
    const int rc = tick_params(a, who, begin, &p);
    if (rc != PWV_OK) return rc;
    if (p.starts) kernel = with_starts;
    const long long floats = ((long long)p.in_frames + p.N) * p.n_mels;
    hipLaunchKernelGGL(kernel, dim3(begin ? (unsigned)((floats + 255) / 256) : 1u), dim3(256), 0, (hipStream_t)stream, p);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

}  // namespace pwv

using namespace pwv;

extern "C" {

int pwv_stream_tick_begin(const pwv_stream_tick_args* a, pwv_stream_t stream) {
    return tick_launch(a, "pwv_stream_tick_begin", true, stream_tick_begin_kernel, stream);
}

int pwv_stream_tick_commit(const pwv_stream_tick_args* a, pwv_stream_t stream) {
    return tick_launch(a, "pwv_stream_tick_commit", false, stream_tick_commit_kernel, stream);
}

int pwv_stream_tick_ragged_begin(const pwv_stream_tick_ragged_args* a, pwv_stream_t stream) {
    return tick_launch(a, "pwv_stream_tick_ragged_begin", true, stream_tick_ragged_begin_kernel, stream, stream_tick_starts_begin_kernel);
}

int pwv_stream_tick_ragged_commit(const pwv_stream_tick_ragged_args* a, pwv_stream_t stream) {
    return tick_launch(a, "pwv_stream_tick_ragged_commit", false, stream_tick_ragged_commit_kernel, stream, stream_tick_starts_commit_kernel);
}

}  // extern "C"
