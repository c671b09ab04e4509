// A streaming tick with its session state on the device (include/pwv_hip.h, "A streaming TICK"): the two small kernels that stand at
// the two ends of a captured push.  stream_tick_begin_kernel turns the session table into the launch tables of the tick (slot table,
// noise streams, the chunk's frames with the kept frame in front); stream_tick_commit_kernel, the tick's last node, advances the
// sessions iff the tick's launches left both sticky words clean.  Plain C++, every address from the arguments, vector stores only.
// stream_tick_ragged_begin_kernel / stream_tick_ragged_commit_kernel are the same pair for a RAGGED tick ("A RAGGED streaming tick"):
// the sessions' frame counts are read from the device too, clamped so that the packed layout is well formed whatever the table holds.
#include <cstddef>

#include "pwv_common.h"

namespace pwv {

struct TickParams {
    long long* sess;
    float* kept;
    const int* entries;
    const float* mel;
    int n_slots, N, frames, n_mels, T;
    int* slot_tab;
    unsigned long long* streams;
    int* cu_rows;
    float* chunk;
    const int* words;
    long long* counters;
};

// entry i as the kernels read it: a slot outside the table is a filler of slot 0 (no address leaves the arrays)
__device__ inline int tick_entry(const TickParams& p, int i, int* live) {
    const int s = p.entries[2 * i];
    const bool ok = (unsigned)s < (unsigned)p.n_slots;
    *live = ok ? p.entries[2 * i + 1] : 0;
    return ok ? s : 0;
}

// one thread per float of chunk [N][frames + 1][n_mels]; the first N + 1 threads also write the tables
__global__ void stream_tick_begin_kernel(TickParams p) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int live;
    if (idx < p.N) {
        const int i = (int)idx, s = tick_entry(p, i, &live);
        const int g = (int)(p.sess[4 * (long long)s] & 1);
        p.slot_tab[2 * i] = 2 * s + g;
        p.slot_tab[2 * i + 1] = 2 * s + 1 - g;
        if (p.streams) {
            p.streams[2 * i] = (unsigned long long)p.sess[4 * (long long)s + 2];
            p.streams[2 * i + 1] = (unsigned long long)p.sess[4 * (long long)s + 1];
            p.cu_rows[i] = i * p.T;
        }
    } else if (idx == p.N && p.cu_rows) {
        p.cu_rows[p.N] = p.N * p.T;
    }
    const int per = (p.frames + 1) * p.n_mels;
    if (idx >= (long long)p.N * per) return;
    const int i = (int)(idx / per), r = (int)(idx % per), f = r / p.n_mels, c = r % p.n_mels;
    const int s = tick_entry(p, i, &live);
    p.chunk[idx] = f == 0 ? p.kept[(long long)s * p.n_mels + c] : p.mel[((long long)i * p.frames + (f - 1)) * p.n_mels + c];
}

// ONE workgroup: the words are read once, so all entries of a tick see one decision
__global__ void stream_tick_commit_kernel(TickParams p) {
    __shared__ int clean;
    if (threadIdx.x == 0) {
        const int gave_up = __hip_atomic_load(p.words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const int range = __hip_atomic_load(p.words + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        clean = (gave_up == 0 && range == 0) ? 1 : 0;
        p.counters[clean ? 0 : 1] += 1;
    }
    __syncthreads();
    if (!clean) return;
    int live;
    for (int i = threadIdx.x; i < p.N; i += blockDim.x) {
        const int s = tick_entry(p, i, &live);
        if (live) {
            p.sess[4 * (long long)s] ^= 1;
            p.sess[4 * (long long)s + 1] += p.T;
        }
    }
    const int total = p.N * p.n_mels;
    for (int k = threadIdx.x; k < total; k += blockDim.x) {
        const int i = k / p.n_mels, c = k % p.n_mels;
        const int s = tick_entry(p, i, &live);
        if (live) p.kept[(long long)s * p.n_mels + c] = p.mel[((long long)i * p.frames + (p.frames - 1)) * p.n_mels + c];
    }
}

// the checks both entry points share: decided before a device is needed
static int tick_params(const pwv_stream_tick_args* a, const char* who, TickParams* p) {
    PWV_CHECK_ARG(a, "%s: args is NULL", who);
    PWV_CHECK_ARG(a->struct_size >= sizeof(pwv_stream_tick_args), "%s: struct_size %zu is short of pwv_stream_tick_args (%zu bytes)", who,
                  a->struct_size, sizeof(pwv_stream_tick_args));
    PWV_CHECK_ARG(a->sess, "%s: sess is NULL", who);
    PWV_CHECK_ARG(a->kept, "%s: kept is NULL", who);
    PWV_CHECK_ARG(a->entries, "%s: entries is NULL", who);
    PWV_CHECK_ARG(a->mel, "%s: mel is NULL", who);
    PWV_CHECK_ARG(a->n_slots >= 1, "%s: n_slots must be >= 1, got %d", who, (int)a->n_slots);
    PWV_CHECK_ARG(a->N >= 1, "%s: N must be >= 1, got %d", who, (int)a->N);
    PWV_CHECK_ARG(a->frames >= 1, "%s: frames must be >= 1, got %d", who, (int)a->frames);
    PWV_CHECK_ARG(a->n_mels >= 1, "%s: n_mels must be >= 1, got %d", who, (int)a->n_mels);
    PWV_CHECK_ARG(a->T >= 1, "%s: T must be >= 1, got %d", who, (int)a->T);
    PWV_CHECK_ARG((long long)a->N * a->T < (1ll << 31) && (long long)a->N * ((long long)a->frames + 1) * a->n_mels < (1ll << 31),
                  "%s: N * T and N * (frames + 1) * n_mels must stay below 2^31", who);
    p->sess = (long long*)a->sess;
    p->kept = a->kept;
    p->entries = a->entries;
    p->mel = a->mel;
    p->n_slots = a->n_slots, p->N = a->N, p->frames = a->frames, p->n_mels = a->n_mels, p->T = a->T;
    p->slot_tab = a->slot_tab;
    p->streams = (unsigned long long*)a->streams;
    p->cu_rows = a->cu_rows;
    p->chunk = a->chunk;
    p->words = a->words;
    p->counters = (long long*)a->counters;
    return PWV_OK;
}

// ---- the RAGGED tick (include/pwv_hip.h, "A RAGGED streaming tick"): every session its own frame count, read from the device ----------

constexpr int RAGGED_MAX_N = 1024;

struct RaggedTickParams {
    long long* sess;
    float* kept;
    const int* entries;
    const float* mel;
    int n_slots, N, in_frames, n_mels, hop, min_frames;
    int* slot_tab;
    unsigned long long* streams;
    int* cu_rows;
    int* cu_frames;
    float* chunk;
    const int* words;
    long long* counters;
};

// The frame counts as the device reads them, by every workgroup for itself: cu[0 .. N] (prefix sums of the clamped counts, cu[N] =
// in_frames), slot[0 .. N-1] and, for the commit, live[0 .. N-1] (a slot outside the table: a filler of slot 0) in LDS.  Whatever `entries` holds,
// cu rises by at least min_frames per entry and ends at in_frames: no address derived from it leaves the arrays.  live: nullptr where the
// caller does not commit (the begin kernel).
__device__ inline void ragged_prefix(const RaggedTickParams& p, int* cu, int* slot, int* live) {
    for (int i = threadIdx.x; i < p.N; i += blockDim.x) {
        const int s = p.entries[4 * i];
        const bool ok = (unsigned)s < (unsigned)p.n_slots;
        slot[i] = ok ? s : 0;
        if (live) live[i] = ok ? p.entries[4 * i + 1] : 0;
        cu[i + 1] = p.entries[4 * i + 2];          // (the wanted count, replaced by the prefix sum below)
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int at = 0;
        cu[0] = 0;
        for (int i = 0; i < p.N - 1; ++i) {
            const int most = p.in_frames - at - (p.N - 1 - i) * p.min_frames;      // >= min_frames: in_frames >= N * min_frames
            const int want = cu[i + 1];
            at += want < p.min_frames ? p.min_frames : (want > most ? most : want);
            cu[i + 1] = at;
        }
        cu[p.N] = p.in_frames;
    }
    __syncthreads();
}

// one thread per float of chunk [in_frames + N][n_mels]; workgroup 0 also writes the tables
__global__ void stream_tick_ragged_begin_kernel(RaggedTickParams p) {
    __shared__ int cu[RAGGED_MAX_N + 1], slot[RAGGED_MAX_N];
    ragged_prefix(p, cu, slot, nullptr);
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i <= p.N; i += blockDim.x) {
            p.cu_rows[i] = p.hop * cu[i];
            p.cu_frames[i] = cu[i] + i;
            if (i == p.N) break;
            const int s = slot[i];
            const int g = (int)(p.sess[4 * (long long)s] & 1);
            p.slot_tab[2 * i] = 2 * s + g;
            p.slot_tab[2 * i + 1] = 2 * s + 1 - g;
            if (p.streams) {
                p.streams[2 * i] = (unsigned long long)p.sess[4 * (long long)s + 2];
                p.streams[2 * i + 1] = (unsigned long long)p.sess[4 * (long long)s + 1];
            }
        }
    }
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)(p.in_frames + p.N) * p.n_mels) return;
    const int row = (int)(idx / p.n_mels), c = (int)(idx % p.n_mels);
    // the session of chunk row `row`: the last i with cu[i] + i <= row (cu[i] + i rises strictly; cu[0] + 0 = 0 <= row)
    int lo = 0, hi = p.N - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (cu[mid] + mid <= row) lo = mid; else hi = mid - 1;
    }
    const int f = row - (cu[lo] + lo);          // 0 .. f_lo: row < cu[lo + 1] + lo + 1
    p.chunk[idx] = f == 0 ? p.kept[(long long)slot[lo] * p.n_mels + c] : p.mel[(long long)(cu[lo] + f - 1) * p.n_mels + c];
}

// ONE workgroup: the words are read once, so all entries of a tick see one decision
__global__ void stream_tick_ragged_commit_kernel(RaggedTickParams p) {
    __shared__ int cu[RAGGED_MAX_N + 1], slot[RAGGED_MAX_N], live[RAGGED_MAX_N];
    __shared__ int clean;
    if (threadIdx.x == 0) {
        const int gave_up = __hip_atomic_load(p.words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const int range = __hip_atomic_load(p.words + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        clean = (gave_up == 0 && range == 0) ? 1 : 0;
        p.counters[clean ? 0 : 1] += 1;
    }
    ragged_prefix(p, cu, slot, live);          // (its barriers publish `clean` too)
    if (!clean) return;
    for (int i = threadIdx.x; i < p.N; i += blockDim.x) {
        if (live[i]) {
            const int s = slot[i];
            p.sess[4 * (long long)s] ^= 1;
            p.sess[4 * (long long)s + 1] += (long long)p.hop * (cu[i + 1] - cu[i]);
        }
    }
    const int total = p.N * p.n_mels;
    for (int k = threadIdx.x; k < total; k += blockDim.x) {
        const int i = k / p.n_mels, c = k % p.n_mels;
        if (live[i]) p.kept[(long long)slot[i] * p.n_mels + c] = p.mel[(long long)(cu[i + 1] - 1) * p.n_mels + c];
    }
}

// the checks both ragged entry points share: decided before a device is needed
static int ragged_tick_params(const pwv_stream_tick_ragged_args* a, const char* who, RaggedTickParams* p) {
    PWV_CHECK_ARG(a, "%s: args is NULL", who);
    PWV_CHECK_ARG(a->struct_size >= sizeof(pwv_stream_tick_ragged_args), "%s: struct_size %zu is short of pwv_stream_tick_ragged_args (%zu bytes)",
                  who, a->struct_size, sizeof(pwv_stream_tick_ragged_args));
    PWV_CHECK_ARG(a->sess, "%s: sess is NULL", who);
    PWV_CHECK_ARG(a->kept, "%s: kept is NULL", who);
    PWV_CHECK_ARG(a->entries, "%s: entries is NULL", who);
    PWV_CHECK_ARG(a->mel, "%s: mel is NULL", who);
    PWV_CHECK_ARG(a->n_slots >= 1, "%s: n_slots must be >= 1, got %d", who, (int)a->n_slots);
    PWV_CHECK_ARG(a->N >= 1 && a->N <= RAGGED_MAX_N, "%s: N must be 1 .. %d, got %d", who, RAGGED_MAX_N, (int)a->N);
    PWV_CHECK_ARG(a->n_mels >= 1, "%s: n_mels must be >= 1, got %d", who, (int)a->n_mels);
    PWV_CHECK_ARG(a->hop >= 1, "%s: hop must be >= 1, got %d", who, (int)a->hop);
    PWV_CHECK_ARG(a->min_frames >= 1, "%s: min_frames must be >= 1, got %d", who, (int)a->min_frames);
    PWV_CHECK_ARG((long long)a->in_frames >= (long long)a->N * a->min_frames, "%s: in_frames must be >= N * min_frames = %lld, got %d", who,
                  (long long)a->N * a->min_frames, (int)a->in_frames);
    PWV_CHECK_ARG((long long)a->in_frames * a->hop < (1ll << 31) && ((long long)a->in_frames + a->N) * a->n_mels < (1ll << 31),
                  "%s: in_frames * hop and (in_frames + N) * n_mels must stay below 2^31", who);
    p->sess = (long long*)a->sess;
    p->kept = a->kept;
    p->entries = a->entries;
    p->mel = a->mel;
    p->n_slots = a->n_slots, p->N = a->N, p->in_frames = a->in_frames, p->n_mels = a->n_mels, p->hop = a->hop, p->min_frames = a->min_frames;
    p->slot_tab = a->slot_tab;
    p->streams = (unsigned long long*)a->streams;
    p->cu_rows = a->cu_rows;
    p->cu_frames = a->cu_frames;
    p->chunk = a->chunk;
    p->words = a->words;
    p->counters = (long long*)a->counters;
    return PWV_OK;
}

}  // namespace pwv

using namespace pwv;

extern "C" {

int pwv_stream_tick_begin(const pwv_stream_tick_args* a, pwv_stream_t stream) {
    TickParams p{};
    const int rc = tick_params(a, "pwv_stream_tick_begin", &p);
    if (rc != PWV_OK) return rc;
    PWV_CHECK_ARG(a->slot_tab, "pwv_stream_tick_begin: slot_tab is NULL");
    PWV_CHECK_ARG(a->chunk, "pwv_stream_tick_begin: chunk is NULL");
    PWV_CHECK_ARG((a->streams == nullptr) == (a->cu_rows == nullptr), "pwv_stream_tick_begin: streams and cu_rows go together (both or neither)");
    const long long floats = (long long)a->N * (a->frames + 1) * a->n_mels;      // > N + 1: frames + 1 >= 2
    hipLaunchKernelGGL(stream_tick_begin_kernel, dim3((unsigned)((floats + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

int pwv_stream_tick_commit(const pwv_stream_tick_args* a, pwv_stream_t stream) {
    TickParams p{};
    const int rc = tick_params(a, "pwv_stream_tick_commit", &p);
    if (rc != PWV_OK) return rc;
    PWV_CHECK_ARG(a->words, "pwv_stream_tick_commit: words is NULL");
    PWV_CHECK_ARG(a->counters, "pwv_stream_tick_commit: counters is NULL");
    hipLaunchKernelGGL(stream_tick_commit_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, p);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

int pwv_stream_tick_ragged_begin(const pwv_stream_tick_ragged_args* a, pwv_stream_t stream) {
    RaggedTickParams p{};
    const int rc = ragged_tick_params(a, "pwv_stream_tick_ragged_begin", &p);
    if (rc != PWV_OK) return rc;
    PWV_CHECK_ARG(a->slot_tab, "pwv_stream_tick_ragged_begin: slot_tab is NULL");
    PWV_CHECK_ARG(a->cu_rows, "pwv_stream_tick_ragged_begin: cu_rows is NULL (required with or without streams: the launches' layout)");
    PWV_CHECK_ARG(a->cu_frames, "pwv_stream_tick_ragged_begin: cu_frames is NULL");
    PWV_CHECK_ARG(a->chunk, "pwv_stream_tick_ragged_begin: chunk is NULL");
    const long long floats = ((long long)a->in_frames + a->N) * a->n_mels;
    hipLaunchKernelGGL(stream_tick_ragged_begin_kernel, dim3((unsigned)((floats + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

int pwv_stream_tick_ragged_commit(const pwv_stream_tick_ragged_args* a, pwv_stream_t stream) {
    RaggedTickParams p{};
    const int rc = ragged_tick_params(a, "pwv_stream_tick_ragged_commit", &p);
    if (rc != PWV_OK) return rc;
    PWV_CHECK_ARG(a->words, "pwv_stream_tick_ragged_commit: words is NULL");
    PWV_CHECK_ARG(a->counters, "pwv_stream_tick_ragged_commit: counters is NULL");
    hipLaunchKernelGGL(stream_tick_ragged_commit_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, p);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

}  // extern "C"
