// One frame of the mel front-end, from its windowed samples to the raw dB of every mel band: the ONE text of the arithmetic, included
// into stft_mel_kernel (the one-shot), stft_mel_stream_kernel and live_tick_mel_kernel (csrc/pwv_audio.hip) so that a streamed frame is
// the one-shot's frame bit for bit.  The kernels differ in how a sample is fetched and in what becomes of the raw dB, nothing else.
//
// The including kernel provides, in scope:
//   double *fr, *ct, *st, *mag      the LDS arrays [n_fft], [n_fft], [n_fft], [n_fft / 2 + 1]
//   const float *window, *fb;  int n_fft, n_mels;  float amin
//   PWV_MEL_FETCH(i)                the float sample under window position i (0 .. n_fft - 1) of this workgroup's frame
//   PWV_MEL_STORE(m, raw)           what to do with band m's raw dB (a float)
// 256 threads; every thread runs the whole text (it holds __syncthreads).
{
    for (int i = threadIdx.x; i < n_fft; i += 256) {
        fr[i] = (double)(PWV_MEL_FETCH(i)) * (double)window[i];
        double s, c;
        sincospi(2.0 * i / n_fft, &s, &c);
        ct[i] = c;
        st[i] = s;
    }
    __syncthreads();
    const int bins = n_fft / 2 + 1;
    for (int b = threadIdx.x; b < bins; b += 256) {
        double re = 0.0, im = 0.0;
        int k = 0;                              // (b * i) mod n_fft
        for (int i = 0; i < n_fft; ++i) {
            re = fma(fr[i], ct[k], re);
            im = fma(fr[i], st[k], im);
            k += b;
            if (k >= n_fft) k -= n_fft;
        }
        mag[b] = sqrt(re * re + im * im);
    }
    __syncthreads();
    for (int m = threadIdx.x; m < n_mels; m += 256) {
        double acc = 0.0;
        const float* row = fb + (size_t)m * bins;
        for (int b = 0; b < bins; ++b) acc = fma((double)row[b], mag[b], acc);
        const double p = acc * acc, floor = (double)amin * (double)amin;
        const float raw = (float)(10.0 * log10(p > floor ? p : floor));
        PWV_MEL_STORE(m, raw);
    }
}
