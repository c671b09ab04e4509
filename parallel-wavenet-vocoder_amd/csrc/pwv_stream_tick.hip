// A streaming tick with its session state on the device (include/pwv_hip.h, "A streaming TICK"): the two small kernels that stand at
// the two ends of a captured push.  stream_tick_begin_kernel turns the session table into the launch tables of the tick (slot table,
// noise streams, the chunk's frames with the kept frame in front); stream_tick_commit_kernel, the tick's last node, advances the
// sessions iff the tick's launches left both sticky words clean.  Plain C++, every address from the arguments, vector stores only.
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

}  // extern "C"
