// wav -> normalised dB mel-spectrogram on the device: the input side of generate.py.
// Restates /root/reference/data_load.py:51-54 with audio.py:102-141 (librosa.stft: centred, reflect-padded, hann window of
// win_length zero-padded to n_fft), :232-243 (Slaney mel filterbank, passed in by the host), :327-356 (amplitude_to_db:
// amin 1e-5, top_db 80 below the utterance maximum) and :254-286 (normalise to [-1, 1]).
// A few hundred MFLOP per utterance: one workgroup per frame, a direct real DFT with fp64 accumulation (the dB scale
// turns relative errors of small bins into absolute ones, so the transform is done in the precision the numpy
// restatement uses), twiddles from an LDS table.  Not a hot path; it exists so that generate() on wav input keeps the mel
// on the device.  The STREAMING form (stft_mel_stream_kernel, pwv_wav_to_mel_db_stream_f32) emits the same frames, bit for bit, from wav
// chunks as they arrive: both kernels include one text of the frame arithmetic, pwv_mel_frame_body.inc.
// The LIVE tick (live_tick_mel_kernel, live_tick_commit_kernel; include/pwv_hip_live_tick.h) is the streaming form at a fixed capacity, for a
// captured graph: records and a front-end session table in device memory, the frames straight into a ragged streaming tick's mel, and
// a commit on the device behind the vocoder's.  It includes the same text.
#include "pwv_common.h"
#include "pwv_hip_live_tick.h"

namespace pwv {

constexpr int kMaxFft = 2048;

// np.pad(mode='reflect') around [0, L): -k -> k, L-1+k -> L-1-k, then clamped (a frame of a short utterance can reach past the mirror)
template <typename I>
__device__ __forceinline__ I reflect_index(I t, I L) {
    if (t < 0) t = -t;
    if (t >= L) t = 2 * (L - 1) - t;
    return t < 0 ? 0 : (t >= L ? L - 1 : t);
}

// (clip((db - min)/(max - min), 0, 1) - .5) * 2: the one fp32 expression of both normalisations
__device__ __forceinline__ float normalise_db(float v, float max_db, float min_db) {
    v = (v - min_db) / (max_db - min_db);
    return (fminf(fmaxf(v, 0.f), 1.f) - 0.5f) * 2.f;
}

// db_raw[n, frame, m] = 10 log10(max(amin^2, mel^2)),  mel = fb[m, :] . |rfft(window * frame)|
__global__ __launch_bounds__(256) void stft_mel_kernel(const float* __restrict__ wav, const float* __restrict__ window,
                                                        const float* __restrict__ fb, float* __restrict__ db, int L, int n_fft,
                                                        int hop, int frames, int n_mels, float amin) {
    extern __shared__ double sm[];             // [n_fft] frame, [n_fft] cos, [n_fft] sin, [n_fft/2 + 1] magnitude
    double* fr = sm;
    double* ct = sm + n_fft;
    double* st = ct + n_fft;
    double* mag = st + n_fft;
    const int f = blockIdx.x, n = blockIdx.y;
    const float* w = wav + (size_t)n * L;
    float* out = db + ((size_t)n * frames + f) * n_mels;
#define PWV_MEL_FETCH(i) w[reflect_index(f * hop + (i) - n_fft / 2, L)]       // centred frame
#define PWV_MEL_STORE(m, raw) out[m] = (raw)
#include "pwv_mel_frame_body.inc"
#undef PWV_MEL_FETCH
#undef PWV_MEL_STORE
}

// ---- the STREAMING form (include/pwv_hip_mel_stream.h) ----
constexpr int kMelRec = PWV_MEL_STREAM_REC;
// a session's record, int64 each
enum { kRecCarryFirst = 0, kRecCarryLen, kRecChunkOff, kRecChunkLen, kRecFirstFrame, kRecFrames, kRecFinalLen, kRecReadBlock, kRecWriteBlock,
       kRecOutRow, kRecNewCarryFirst, kRecMaxWord };

// an integer key that orders as the floats do (no NaN reaches it: the dB of a NaN power is the amin floor's)
__device__ __forceinline__ int float_key(float v) {
    const int b = __float_as_int(v);
    return b >= 0 ? b : b ^ 0x7fffffff;
}

// Sample `t` (absolute, already mirrored) of a session that holds samples c0 .. c0 + clen - 1 in `carry` and the next `chlen` in `chunk`.
// The host has checked that every index a launch asks for lies inside the two; the clamp keeps a wrong record inside them as well.
__device__ __forceinline__ float stream_sample(const float* __restrict__ carry, const float* __restrict__ chunk, long long t, long long c0,
                                               long long clen, long long chlen) {
    long long p = t - c0;
    p = p < 0 ? 0 : (p >= clen + chlen ? clen + chlen - 1 : p);
    return p < clen ? carry[p] : chunk[p - clen];
}

// the sample index frame position t reads: the one-shot's mirrors once the final length L is known, else (L < 0) the left one alone
__device__ __forceinline__ long long stream_index(long long t, long long L) { return L >= 0 ? reflect_index(t, L) : (t < 0 ? -t : t); }

// One workgroup per (frame, session) of a ragged push: blockIdx.y = session, blockIdx.x = 0 .. frames - 1 a frame of it (normalised, the
// session's largest raw dB kept in its max word), blockIdx.x == frames the session's new carry, beyond that nothing.
__global__ __launch_bounds__(256) void stft_mel_stream_kernel(const float* __restrict__ wav, const float* __restrict__ window,
                                                               const float* __restrict__ fb, float* __restrict__ mel, float* state,
                                                               int* __restrict__ max_key, const long long* __restrict__ rec, int n_fft,
                                                               int hop, int n_mels, float amin, float max_db, float min_db) {
    extern __shared__ double sm[];             // as stft_mel_kernel
    __shared__ int wg_max;
    double* fr = sm;
    double* ct = sm + n_fft;
    double* st = ct + n_fft;
    double* mag = st + n_fft;
    const long long* r = rec + (size_t)blockIdx.y * kMelRec;
    const long long frames = r[kRecFrames], L = r[kRecFinalLen];
    if ((long long)blockIdx.x > frames) return;
    const long long c0 = r[kRecCarryFirst], clen = r[kRecCarryLen], chlen = r[kRecChunkLen];
    const float* carry = state + (size_t)r[kRecReadBlock] * n_fft;
    const float* chunk = wav + r[kRecChunkOff];
    if ((long long)blockIdx.x == frames) {
        if (L >= 0) return;                    // a finished utterance carries nothing on
        float* next = state + (size_t)r[kRecWriteBlock] * n_fft;       // (another block than `carry`: two generations)
        const long long c1 = r[kRecNewCarryFirst], keep = c0 + clen + chlen - c1;
        for (long long i = threadIdx.x; i < keep && i < n_fft; i += 256) next[i] = stream_sample(carry, chunk, c1 + i, c0, clen, chlen);
        return;
    }
    const long long f = r[kRecFirstFrame] + blockIdx.x;
    float* out = mel + (size_t)(r[kRecOutRow] + blockIdx.x) * n_mels;
    if (threadIdx.x == 0) wg_max = float_key(-3.0e38f);               // (the body's first barrier orders it)
    // before `finish` no frame reads at or beyond R (the ready rule), so only the left mirror applies; at `finish` both, as in the one-shot
#define PWV_MEL_FETCH(i) stream_sample(carry, chunk, stream_index(f * hop + (i) - n_fft / 2, L), c0, clen, chlen)
#define PWV_MEL_STORE(m, raw)                          \
    do {                                               \
        out[m] = normalise_db((raw), max_db, min_db);  \
        atomicMax(&wg_max, float_key(raw));            \
    } while (0)
#include "pwv_mel_frame_body.inc"
#undef PWV_MEL_FETCH
#undef PWV_MEL_STORE
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(max_key + r[kRecMaxWord], wg_max);
}

// ---- the LIVE tick (include/pwv_hip_live_tick.h): the capacity form of the streaming kernel and the front-end commit ----
constexpr int kLiveRec = PWV_LIVE_TICK_REC;
enum { kLiveSlot = 7, kLiveFlags = 8, kLiveFirstRow = 11 };       // (the other fields are the streaming record's)
enum { kLiveActive = 1, kLiveStart = 2, kLiveFirst = 4 };
constexpr int kKeyNone = -2147483647 - 1;

struct LiveParams {
    const float* wav;
    const float* window;
    const float* fb;
    float* mel;
    float* first;
    float* state;
    int* max_key;
    int* scratch;
    long long* sess;
    const long long* rec;
    const int* words;
    long long wav_cap, mel_rows;
    int N, n_slots, n_first, n_fft, hop, n_mels;
    float amin, max_db, min_db, limit_db;
};

// Record i as both kernels read it: every value clamped to what the call was given, whatever the table holds.
struct LiveRecord {
    long long c0, clen, coff, chlen, first, frames, L, c1, row, first_row;
    int slot, flags;
    bool active;
};

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ LiveRecord live_record(const LiveParams& p, int i) {
    const long long* r = p.rec + (size_t)i * kLiveRec;
    LiveRecord q;
    q.flags = (int)r[kLiveFlags];
    const long long slot = r[kLiveSlot];
    q.active = (q.flags & kLiveActive) != 0 && slot >= 0 && slot < p.n_slots;
    q.slot = q.active ? (int)slot : 0;
    q.c0 = clampll(r[kRecCarryFirst], 0, 1ll << 62);
    q.clen = (q.flags & kLiveStart) ? 0 : clampll(r[kRecCarryLen], 0, p.n_fft);        // a start reads no carry
    q.coff = clampll(r[kRecChunkOff], 0, p.wav_cap);
    q.chlen = clampll(r[kRecChunkLen], 0, p.wav_cap - q.coff);
    q.first = clampll(r[kRecFirstFrame], 0, 1ll << 40);
    q.frames = q.clen + q.chlen > 0 ? clampll(r[kRecFrames], 0, p.mel_rows + 1) : 0;   // (no sample held: nothing to read)
    q.L = clampll(r[kRecFinalLen], -1, 1ll << 62);
    q.c1 = clampll(r[kRecNewCarryFirst], 0, 1ll << 62);
    q.row = r[kRecOutRow];
    q.first_row = r[kLiveFirstRow];
    return q;
}

// Workgroup b is frame x of record i, or (x == its frames) its carry: the records' frames + 1 in a row, inactive records none.
// A workgroup behind them all has nothing to do.
__global__ __launch_bounds__(256) void live_tick_mel_kernel(LiveParams p) {
    extern __shared__ double sm[];             // as stft_mel_kernel
    __shared__ int wg_max;
    const int n_fft = p.n_fft, n_mels = p.n_mels;
    const float amin = p.amin;
    const float* window = p.window;
    const float* fb = p.fb;
    double* fr = sm;
    double* ct = sm + n_fft;
    double* st = ct + n_fft;
    double* mag = st + n_fft;
    long long x = blockIdx.x;
    int i = 0;
    for (; i < p.N; ++i) {
        const long long* r = p.rec + (size_t)i * kLiveRec;
        const long long slot = r[kLiveSlot];
        if (!((r[kLiveFlags] & kLiveActive) != 0 && slot >= 0 && slot < p.n_slots)) continue;
        const long long count = clampll(r[kRecFrames], 0, p.mel_rows + 1) + 1;
        if (x < count) break;
        x -= count;
    }
    if (i >= p.N) return;
    const LiveRecord q = live_record(p, i);
    const int g = (int)(p.sess[4 * (long long)q.slot] & 1);
    const float* carry = p.state + (size_t)(2 * q.slot + g) * n_fft;
    const float* chunk = p.wav + q.coff;
    const long long c0 = q.c0, clen = q.clen, chlen = q.chlen, L = q.L;
    if (x >= q.frames) {
        if (x > q.frames || L >= 0 || clen + chlen <= 0) return;      // (a finished utterance carries nothing on)
        float* next = p.state + (size_t)(2 * q.slot + 1 - g) * n_fft;
        const long long keep = c0 + clen + chlen - q.c1;
        for (long long k = threadIdx.x; k < keep && k < n_fft; k += 256) next[k] = stream_sample(carry, chunk, q.c1 + k, c0, clen, chlen);
        return;
    }
    float* out;
    if (q.flags & kLiveFirst) {
        const long long row = x == 0 ? q.first_row : q.row + x - 1;
        if (row < 0 || row >= (x == 0 ? (long long)p.n_first : p.mel_rows)) return;
        out = (x == 0 ? p.first : p.mel) + (size_t)row * n_mels;
    } else {
        const long long row = q.row + x;
        if (row < 0 || row >= p.mel_rows) return;
        out = p.mel + (size_t)row * n_mels;
    }
    const long long f = q.first + x;
    const int hop = p.hop;
    const float max_db = p.max_db, min_db = p.min_db;
    if (threadIdx.x == 0) wg_max = float_key(-3.0e38f);               // (the body's first barrier orders it)
#define PWV_MEL_FETCH(i) stream_sample(carry, chunk, stream_index(f * hop + (i) - n_fft / 2, L), c0, clen, chlen)
#define PWV_MEL_STORE(m, raw)                          \
    do {                                               \
        out[m] = normalise_db((raw), max_db, min_db);  \
        atomicMax(&wg_max, float_key(raw));            \
    } while (0)
#include "pwv_mel_frame_body.inc"
#undef PWV_MEL_FETCH
#undef PWV_MEL_STORE
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(p.scratch + i, wg_max);
}

// ONE workgroup, behind the ragged tick's commit: the words are read once, so all records of a tick see one decision
__global__ __launch_bounds__(256) void live_tick_commit_kernel(LiveParams p) {
    __shared__ int clean;
    if (threadIdx.x == 0) {
        const int gave_up = __hip_atomic_load(p.words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const int range = __hip_atomic_load(p.words + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        clean = (gave_up == 0 && range == 0) ? 1 : 0;
    }
    __syncthreads();
    const int limit = float_key(p.limit_db);
    for (int i = threadIdx.x; i < p.N; i += 256) {
        const int key = p.scratch[i];
        p.scratch[i] = kKeyNone;
        if (!clean) continue;
        const LiveRecord q = live_record(p, i);
        if (!q.active) continue;
        long long* s = p.sess + 4 * (long long)q.slot;
        const bool start = (q.flags & kLiveStart) != 0;
        int word = p.max_key[q.slot];
        word = start || key > word ? key : word;
        s[0] ^= 1;
        if (word > limit) s[3] = 1;
        if (q.L >= 0) {
            s[1] = 0, s[2] = 0;
            word = kKeyNone;
        } else {
            s[1] = (start ? 0 : s[1]) + q.chlen;
            s[2] = (start ? 0 : s[2]) + q.frames;
        }
        p.max_key[q.slot] = word;
    }
}

// per utterance: top_db clip against the maximum of the whole spectrogram, then (clip((db - min)/(max - min), 0, 1) - .5) * 2
__global__ __launch_bounds__(1024) void db_normalize_kernel(float* __restrict__ db, int count, float top_db, float max_db, float min_db,
                                                            int normalise) {
    __shared__ float red[1024];
    float* p = db + (size_t)blockIdx.x * count;
    float mx = -3.0e38f;
    for (int i = threadIdx.x; i < count; i += 1024) mx = fmaxf(mx, p[i]);
    red[threadIdx.x] = mx;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    const float lo = red[0] - top_db;
    for (int i = threadIdx.x; i < count; i += 1024) {
        float v = fmaxf(p[i], lo);
        if (normalise) v = normalise_db(v, max_db, min_db);
        p[i] = v;
    }
}

}  // namespace pwv

using namespace pwv;

extern "C" {

int pwv_wav_to_mel_db_f32(const float* wav, const float* window, const float* mel_basis, float* mel, int N, int L, int n_fft, int hop,
                          int n_mels, float amin, float top_db, float max_db, float min_db, int normalise, pwv_stream_t stream) {
    PWV_CHECK_ARG(wav && window && mel_basis && mel, "pwv_wav_to_mel_db_f32: NULL pointer");
    PWV_CHECK_ARG(N >= 1 && L >= 2 && hop >= 1 && n_mels >= 1, "pwv_wav_to_mel_db_f32: bad shape");
    PWV_CHECK_ARG(n_fft >= 2 && n_fft % 2 == 0 && n_fft <= kMaxFft && n_fft / 2 < L, "pwv_wav_to_mel_db_f32: n_fft must be even, <= %d and < 2 L", kMaxFft);
    PWV_CHECK_ARG(!normalise || max_db != min_db, "pwv_wav_to_mel_db_f32: max_db == min_db");
    const int frames = 1 + L / hop;
    hipStream_t s = (hipStream_t)stream;
    const size_t smem = (size_t)(3 * n_fft + n_fft / 2 + 1) * sizeof(double);
    hipLaunchKernelGGL(stft_mel_kernel, dim3(frames, N), dim3(256), smem, s, wav, window, mel_basis, mel, L, n_fft, hop, frames, n_mels, amin);
    hipLaunchKernelGGL(db_normalize_kernel, dim3(N), dim3(1024), 0, s, mel, frames * n_mels, top_db, max_db, min_db, normalise);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

int pwv_wav_to_mel_db_stream_f32(const pwv_mel_stream_args* a, pwv_stream_t stream) {
    static const char who[] = "pwv_wav_to_mel_db_stream_f32";
    // every refusal stands in front of the launch: nothing below touches a device before the last check has passed
    PWV_CHECK_ARG(a, "%s: args is NULL", who);
    PWV_CHECK_ARG(a->struct_size >= sizeof(pwv_mel_stream_args), "%s: struct_size %zu is short of pwv_mel_stream_args (%zu bytes)", who,
                  a->struct_size, sizeof(pwv_mel_stream_args));
    PWV_CHECK_ARG(a->window, "%s: window is a NULL pointer", who);
    PWV_CHECK_ARG(a->mel_basis, "%s: mel_basis is a NULL pointer", who);
    PWV_CHECK_ARG(a->state, "%s: state is a NULL pointer", who);
    PWV_CHECK_ARG(a->max_key, "%s: max_key is a NULL pointer", who);
    PWV_CHECK_ARG(a->rec && a->rec_host, "%s: rec / rec_host is a NULL pointer", who);
    PWV_CHECK_ARG(a->wav_len >= 0 && (a->wav || a->wav_len == 0), "%s: wav is a NULL pointer (wav_len %lld)", who, (long long)a->wav_len);
    PWV_CHECK_ARG(a->mel_rows >= 0 && (a->mel || a->mel_rows == 0), "%s: mel is a NULL pointer (mel_rows %lld)", who, (long long)a->mel_rows);
    PWV_CHECK_ARG(a->n_fft >= 2 && a->n_fft % 2 == 0 && a->n_fft <= kMaxFft, "%s: n_fft %d must be even, >= 2 and <= %d", who, a->n_fft, kMaxFft);
    PWV_CHECK_ARG(a->hop >= 1, "%s: hop %d must be >= 1", who, a->hop);
    PWV_CHECK_ARG(a->n_mels >= 1, "%s: n_mels %d must be >= 1", who, a->n_mels);
    PWV_CHECK_ARG(a->max_db != a->min_db, "%s: max_db == min_db (the streaming form is the normalised one)", who);
    PWV_CHECK_ARG(a->N >= 1 && a->N <= 65535, "%s: N %d out of range (1 .. 65535 sessions in a push)", who, a->N);
    PWV_CHECK_ARG(a->n_blocks >= 2 && a->n_words >= 1, "%s: n_blocks %d / n_words %d", who, a->n_blocks, a->n_words);
    const long long h = a->n_fft / 2, hop = a->hop;
    long long max_frames = 0;
    for (int i = 0; i < a->N; ++i) {
        const int64_t* r = a->rec_host + (size_t)i * kMelRec;
        const long long c0 = r[kRecCarryFirst], clen = r[kRecCarryLen], coff = r[kRecChunkOff], chlen = r[kRecChunkLen], first = r[kRecFirstFrame],
                        frames = r[kRecFrames], L = r[kRecFinalLen], row = r[kRecOutRow], c1 = r[kRecNewCarryFirst];
        const long long R = c0 + clen + chlen;
        PWV_CHECK_ARG(c0 >= 0 && clen >= 0 && clen <= a->n_fft && c0 <= (1ll << 62), "%s: record %d: carry %lld + %lld", who, i, c0, clen);
        PWV_CHECK_ARG(coff >= 0 && chlen >= 0 && chlen <= a->wav_len && coff <= a->wav_len - chlen, "%s: record %d: chunk %lld + %lld leaves wav_len %lld", who, i,
                      coff, chlen, (long long)a->wav_len);
        PWV_CHECK_ARG(first >= 0 && frames >= 0 && frames < (1ll << 31) - 1 && first <= (1ll << 40), "%s: record %d: frames %lld + %lld", who, i, first, frames);
        PWV_CHECK_ARG(row >= 0 && frames <= a->mel_rows && row <= a->mel_rows - frames, "%s: record %d: rows %lld + %lld leave mel_rows %lld", who, i, row, frames,
                      (long long)a->mel_rows);
        PWV_CHECK_ARG(r[kRecReadBlock] >= 0 && r[kRecReadBlock] < a->n_blocks && r[kRecWriteBlock] >= 0 && r[kRecWriteBlock] < a->n_blocks &&
                          r[kRecReadBlock] != r[kRecWriteBlock],
                      "%s: record %d: read block %lld, written block %lld of %d", who, i, (long long)r[kRecReadBlock], (long long)r[kRecWriteBlock], a->n_blocks);
        PWV_CHECK_ARG(r[kRecMaxWord] >= 0 && r[kRecMaxWord] < a->n_words, "%s: record %d: max word %lld of %d", who, i, (long long)r[kRecMaxWord], a->n_words);
        PWV_CHECK_ARG(L == -1 || L == R, "%s: record %d: final_len %lld is not the %lld samples received", who, i, L, R);
        PWV_CHECK_ARG(L == -1 || L > h, "%s: record %d: final_len %lld must exceed n_fft / 2 = %lld", who, i, L, h);
        if (frames > 0) {
            // the indices the frames read, mirrored as the kernel mirrors them, lie in [c0, R)
            const long long t0 = first * hop - h, t1 = (first + frames - 1) * hop + h - 1;
            const long long a0 = t0 >= 0 ? t0 : (t1 >= 0 ? 0 : -t1), a1 = t0 >= 0 ? t1 : (-t0 > t1 ? -t0 : t1);      // behind the left mirror
            long long lo = a0, hi = a1;
            if (L >= 0) {                      // behind the right mirror and the clamp
                lo = a0 < L ? a0 : L - 1;
                if (a1 >= L) {
                    const long long m = 2 * (L - 1) - a1;
                    if (m < lo) lo = m < 0 ? 0 : m;
                }
                hi = a1 < L ? a1 : L - 1;
            }
            PWV_CHECK_ARG(lo >= c0 && hi < R, "%s: record %d: frames %lld .. %lld read samples %lld .. %lld, held are %lld .. %lld", who, i, first,
                          first + frames - 1, lo, hi, c0, R - 1);
        }
        if (L < 0) PWV_CHECK_ARG(c1 >= c0 && c1 <= R && R - c1 <= a->n_fft, "%s: record %d: new carry %lld .. %lld", who, i, c1, R - 1);
        if (frames > max_frames) max_frames = frames;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t smem = (size_t)(3 * a->n_fft + a->n_fft / 2 + 1) * sizeof(double);
    hipLaunchKernelGGL(stft_mel_stream_kernel, dim3((unsigned)(max_frames + 1), a->N), dim3(256), smem, s, a->wav, a->window, a->mel_basis, a->mel,
                       a->state, a->max_key, (const long long*)a->rec, a->n_fft, a->hop, a->n_mels, a->amin, a->max_db, a->min_db);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

// the live tick: check, then one launch whose grid N and mel_rows alone decide
static int live_params(const pwv_live_tick_args* a, const char* who, LiveParams* p) {
    PWV_CHECK_ARG(a, "%s: args is NULL", who);
    PWV_CHECK_ARG(a->struct_size >= sizeof(pwv_live_tick_args), "%s: struct_size %zu is short of pwv_live_tick_args (%zu bytes)", who,
                  a->struct_size, sizeof(pwv_live_tick_args));
    PWV_CHECK_ARG(a->window, "%s: window is a NULL pointer", who);
    PWV_CHECK_ARG(a->mel_basis, "%s: mel_basis is a NULL pointer", who);
    PWV_CHECK_ARG(a->mel, "%s: mel is a NULL pointer", who);
    PWV_CHECK_ARG(a->state, "%s: state is a NULL pointer", who);
    PWV_CHECK_ARG(a->max_key, "%s: max_key is a NULL pointer", who);
    PWV_CHECK_ARG(a->scratch, "%s: scratch is a NULL pointer", who);
    PWV_CHECK_ARG(a->sess, "%s: sess is a NULL pointer", who);
    PWV_CHECK_ARG(a->rec, "%s: rec is a NULL pointer", who);
    PWV_CHECK_ARG(a->words, "%s: words is a NULL pointer", who);
    PWV_CHECK_ARG(a->wav_cap >= 0 && (a->wav || a->wav_cap == 0), "%s: wav is a NULL pointer (wav_cap %lld)", who, (long long)a->wav_cap);
    PWV_CHECK_ARG(a->n_first >= 0 && (a->first || a->n_first == 0), "%s: first is a NULL pointer (n_first %d)", who, a->n_first);
    PWV_CHECK_ARG(a->n_fft >= 2 && a->n_fft % 2 == 0 && a->n_fft <= kMaxFft, "%s: n_fft %d must be even, >= 2 and <= %d", who, a->n_fft, kMaxFft);
    PWV_CHECK_ARG(a->hop >= 1, "%s: hop %d must be >= 1", who, a->hop);
    PWV_CHECK_ARG(a->n_mels >= 1, "%s: n_mels %d must be >= 1", who, a->n_mels);
    PWV_CHECK_ARG(a->max_db != a->min_db, "%s: max_db == min_db (the streaming form is the normalised one)", who);
    PWV_CHECK_ARG(a->N >= 1 && a->N <= 65535, "%s: N %d out of range (1 .. 65535 records in a tick)", who, a->N);
    PWV_CHECK_ARG(a->n_slots >= 1, "%s: n_slots %d must be >= 1", who, a->n_slots);
    PWV_CHECK_ARG(a->mel_rows >= 1 && a->mel_rows + 2ll * a->N < (1ll << 31), "%s: mel_rows %lld out of range", who, (long long)a->mel_rows);
    for (int i = 0; a->rec_host && i < a->N; ++i) {
        const int64_t* r = a->rec_host + (size_t)i * kLiveRec;
        if (!(r[kLiveFlags] & kLiveActive)) continue;
        const long long clen = r[kRecCarryLen], coff = r[kRecChunkOff], chlen = r[kRecChunkLen], frames = r[kRecFrames], L = r[kRecFinalLen],
                        row = r[kRecOutRow], in_mel = frames - ((r[kLiveFlags] & kLiveFirst) && frames > 0 ? 1 : 0);
        PWV_CHECK_ARG(r[kRecCarryFirst] >= 0 && clen >= 0 && clen <= a->n_fft, "%s: record %d: carry %lld + %lld", who, i, (long long)r[kRecCarryFirst], clen);
        PWV_CHECK_ARG(coff >= 0 && chlen >= 0 && chlen <= a->wav_cap && coff <= a->wav_cap - chlen, "%s: record %d: chunk %lld + %lld leaves wav_cap %lld",
                      who, i, coff, chlen, (long long)a->wav_cap);
        PWV_CHECK_ARG(r[kRecFirstFrame] >= 0 && frames >= 0 && row >= 0 && in_mel <= a->mel_rows && row <= a->mel_rows - in_mel,
                      "%s: record %d: rows %lld + %lld leave mel_rows %lld", who, i, row, in_mel, (long long)a->mel_rows);
        PWV_CHECK_ARG(r[kLiveSlot] >= 0 && r[kLiveSlot] < a->n_slots, "%s: record %d: slot %lld has no state blocks (n_slots %d)", who, i,
                      (long long)r[kLiveSlot], a->n_slots);
        PWV_CHECK_ARG(!(r[kLiveFlags] & kLiveFirst) || (r[kLiveFirstRow] >= 0 && r[kLiveFirstRow] < a->n_first),
                      "%s: record %d: first row %lld is outside the %d words / rows of first", who, i, (long long)r[kLiveFirstRow], a->n_first);
        PWV_CHECK_ARG(L == -1 || L > a->n_fft / 2, "%s: record %d: final_len %lld must exceed n_fft / 2 = %d", who, i, L, a->n_fft / 2);
    }
    *p = LiveParams{a->wav, a->window, a->mel_basis, a->mel, a->first, a->state, a->max_key, a->scratch, (long long*)a->sess, (const long long*)a->rec,
                    a->words, a->wav_cap, a->mel_rows, a->N, a->n_slots, a->n_first, a->n_fft, a->hop, a->n_mels, a->amin, a->max_db, a->min_db,
                    a->limit_db};
    return PWV_OK;
}

int pwv_live_tick_mel(const pwv_live_tick_args* a, pwv_stream_t stream) {
    LiveParams p{};
    const int rc = live_params(a, "pwv_live_tick_mel", &p);
    if (rc != PWV_OK) return rc;
    const size_t smem = (size_t)(3 * p.n_fft + p.n_fft / 2 + 1) * sizeof(double);
    hipLaunchKernelGGL(live_tick_mel_kernel, dim3((unsigned)(p.mel_rows + 2 * p.N)), dim3(256), smem, (hipStream_t)stream, p);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

int pwv_live_tick_commit(const pwv_live_tick_args* a, pwv_stream_t stream) {
    LiveParams p{};
    const int rc = live_params(a, "pwv_live_tick_commit", &p);
    if (rc != PWV_OK) return rc;
    hipLaunchKernelGGL(live_tick_commit_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, p);
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

}  // extern "C"
