// wav -> normalised dB mel-spectrogram on the device: the input side of generate.py.
// Restates /root/reference/data_load.py:51-54 with audio.py:102-141 (librosa.stft: centred, reflect-padded, hann window of
// win_length zero-padded to n_fft), :232-243 (Slaney mel filterbank, passed in by the host), :327-356 (amplitude_to_db:
// amin 1e-5, top_db 80 below the utterance maximum) and :254-286 (normalise to [-1, 1]).
// A few hundred MFLOP per utterance: one workgroup per frame, a direct real DFT with fp64 accumulation (the dB scale
// turns relative errors of small bins into absolute ones, so the transform is done in the precision the numpy
// restatement uses), twiddles from an LDS table.  Not a hot path; it exists so that generate() on wav input keeps the mel
// on the device.  The STREAMING form (stft_mel_stream_kernel, pwv_wav_to_mel_db_stream_f32) emits the same frames, bit for bit, from wav
// chunks as they arrive: both kernels include one text of the frame arithmetic, pwv_mel_frame_body.inc.
#include "pwv_common.h"
#include "pwv_hip_mel_stream.h"

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

}  // extern "C"
