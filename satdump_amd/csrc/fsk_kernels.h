// fsk_kernels.h -- the REAL-VALUED demodulator chain of fsk_demod / sdpsk_demod on gfx950 (wave64): what follows BaseDemodModule's complex AGC in
// module_fsk_demod.cpp:59-84 and module_sdpsk_demod.cpp:56-71 --
//   QuadratureDemodBlock (quadrature_demod.cpp:36-48) -> CorrectIQBlock<float> (correct_iq.cpp:27-31) -> [fsk only] AGCBlock<float>(0.1, 0.5, 1, 65535)
//   (agc.cpp:25-39, the fabsf branch) -> FIRBlock<float> (fir.cpp:59-71) -> MMClockRecoveryBlock<float> (clock_recovery_mm.cpp:70-88,111-120) -> clamp(sym * scale).
//
// Declarations for the engine, and -- where SDHIP_FSK_KERNELS_IMPL is defined, at the end of demod_kernels.hip -- the kernels with their launch functions.
//
// Every stage has ONE kernel for both modes of the engine: the library is compiled without contraction, each float operation below is rounded where the
// reference rounds it, and what distinguishes the modes is the schedule alone.
//   * The quadrature demodulator and the FIR have no state beyond their input window: a thread per sample, the reference's operations in its order --
//     their output is the reference's bit for bit in either mode.
//   * The DC block, the float AGC and the clock recovery are recurrences: a lane per chunk (ChunkGeom). exact = 1 is the geometry with one chunk: one sequential
//     lane. exact = 0: the DC block's chunk start values come from an affine scan in double (k_fdc_partial + the host's chain, as for the complex DC block),
//     the AGC's and the clock recovery's from a warm-up in front of the chunk; the engine's certificates decide what stands (DemodEngine::fsk_tail).
// The lanes read and write their chunks as float4 (16 bytes per request and lane): per-lane requests bound these stages; they are kept
// simple here -- no cooperative loads -- because the chain's cost sits in the clock recovery's dependent chain per symbol, not in its traffic.
#pragma once
#include "demod_kernels.h"

namespace sdhip
{
    constexpr int FSK_HIST = 512; // floats of history kept in front of the FIR's and the clock recovery's input (>= ntaps - 1, >= 7)

    struct FagcParams
    {
        float rate, reference, max_gain, init_gain;
    };
    // MMClockRecoveryBlock<float>: the complex block's loop with the detector sign(last) * s - sign(s) * last on ONE delayed sample
    struct FmmParams
    {
        float omega_gain, mu_gain, omega_mid, omega_limit, init_mu;
        const float *bank; // [128][8] device (design::mm_bank)
        int cap;           // symbols per scratch row
        int fast_syms;     // warm-up gear shift as in MmParams
        float fast_mult;
    };
    struct FmmState
    {
        float mu, omega, last;
        int pad;
        long long inc;
    };

    // y[i] = wrap(atan2f(x[i]) - atan2f(x[i - 1])) * gain; the angle in front of x[0] is *phase_in, the last one goes to *phase_out (two different words)
    void launch_fquad(const cf32 *x, float *y, long long n, float gain, const float *phase_in, float *phase_out, hipStream_t st);
    // CorrectIQBlock<float>: DcState::acc_re carries the accumulator (acc_im = 0). partial: one double per chunk, B_k = sum beta^(len - 1 - i) alpha x_i.
    // launch_fdc: chunk k starts from starts[k]; redo lanes from spec[k] (the engine put the predecessor's end state there)
    void launch_fdc_partial(const float *x, const ChunkGeom &g, double *partial, hipStream_t st);
    void launch_fdc(const float *x, float *y, const ChunkGeom &g, const DcState *starts, DcState *spec, DcState *endst, const int *redo, int nredo, hipStream_t st);
    // AGCBlock<float>: chunk 0 starts from *start0, the others warm up over g.W samples from init_gain
    void launch_fagc(const float *x, float *y, const ChunkGeom &g, const FagcParams &p, const AgcState *start0, AgcState *spec, AgcState *endst, const int *redo, int nredo,
                     hipStream_t st);
    // y[i] = sum_j x[i - (ntaps - 1) + j] * rtaps[j], j ascending from 0.0f (x[-1 .. -(ntaps - 1)]: the history in front of the buffer); ntaps <= FSK_HIST
    void launch_ffir(const float *x, float *y, long long n, const float *rtaps_dev, int ntaps, hipStream_t st);
    // counts / spec_c / end_c as launch_mm's (k_mm_verdict and the chunk scan serve both); rows = K x cap floats
    void launch_fmm(const float *x, float *rows, int *counts, const ChunkGeom &g, const FmmParams &p, const FmmState *start0, FmmState *spec, FmmState *endst, MmCert *spec_c,
                    MmCert *end_c, const int *redo, int nredo, hipStream_t st);
    // compaction of the rows (seg / offsets from the chunk scan) + clamp(sym * scale): ONE int8 and, if syms != nullptr, ONE float per symbol
    void launch_fquant(const float *rows, const int *seg, const long long *offsets, int K, int cap, float scale, int8_t *soft, long long soft_cap, float *syms,
                       long long syms_cap, hipStream_t st);
    // partial[b] (64 doubles) = sum |x[i]| over block b's share of x[0 .. n): the level the clock recovery's detector gain goes with
    void launch_fmean_abs(const float *x, long long n, double *partial, hipStream_t st);
    // hist <- the last FSK_HIST floats of [hist | cur[0 .. ncur)]
    void launch_fhist_slide(float *hist, const float *cur, long long ncur, hipStream_t st);

#ifdef SDHIP_FSK_KERNELS_IMPL
    __global__ __launch_bounds__(256) void k_fquad(const cf32 *x, float *y, long long n, float gain, const float *phase_in, float *phase_out)
    {
        const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n)
            return;
        const cf32 v = x[i];
        const float p = s2_atan2f(v.im, v.re);
        float prev;
        if (i > 0)
        { // the previous sample's angle is recomputed: the stage's only state
            const cf32 u = x[i - 1];
            prev = s2_atan2f(u.im, u.re);
        }
        else
            prev = *phase_in;
        float d = p - prev;
        // (M_PI is a double: the comparison and the correction happen in double, the result narrows to the float member)
        const double pi = 3.14159265358979323846;
        if ((double)d > pi)
            d = (float)((double)d - (double)2.0f * pi);
        else if ((double)d <= -pi)
            d = (float)((double)d + (double)2.0f * pi);
        y[i] = d * gain;
        if (i == n - 1)
            *phase_out = p;
    }

    __global__ __launch_bounds__(256) void k_fdc_partial(const float *x, ChunkGeom g, double *partial)
    {
        __shared__ double acc[256];
        const int k = (int)blockIdx.x, t = (int)threadIdx.x;
        const long long b = chunk_begin(g, k), e = chunk_end(g, k);
        const long long seg = (e - b + 255) / 256;
        const long long s0 = b + (long long)t * seg, s1 = s0 + seg < e ? s0 + seg : e;
        const double alpha = (double)0.0001f, beta = (double)(1.0f - 0.0001f);
        double v = 0.0;
        for (long long i = s0; i < s1; i++)
            v = v * beta + alpha * (double)x[i];
        acc[t] = s0 < s1 ? v * pow(beta, (double)(e - s1)) : 0.0;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1)
        {
            if (t < s)
                acc[t] += acc[t + s];
            __syncthreads();
        }
        if (t == 0)
            partial[k] = acc[0];
    }

    // the body of a lane over [from, to): float4 groups while they fit (the chunk limits are multiples of 8 samples but for the stream's end), then sample by sample
    template <class F>
    __device__ __forceinline__ void flane_walk(const float *x, float *y, long long from, const long long to, F &&step)
    {
        for (; from + 4 <= to; from += 4)
        {
            const float4 v = *reinterpret_cast<const float4 *>(x + from);
            float4 o;
            o.x = step(v.x);
            o.y = step(v.y);
            o.z = step(v.z);
            o.w = step(v.w);
            if (y)
                *reinterpret_cast<float4 *>(y + from) = o;
        }
        for (; from < to; from++)
        {
            const float o = step(x[from]);
            if (y)
                y[from] = o;
        }
    }

    __global__ __launch_bounds__(64) void k_fdc(const float *x, float *y, ChunkGeom g, const DcState *starts, DcState *spec, DcState *endst, const int *redo, int nredo)
    {
        const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
        int k;
        float acc;
        if (redo)
        {
            if (idx >= nredo)
                return;
            k = redo[idx];
            acc = spec[k].acc_re;
        }
        else
        {
            k = idx;
            if (k >= g.K)
                return;
            acc = starts[k].acc_re;
            spec[k] = DcState{acc, 0.0f};
        }
        const float alpha = 0.0001f, beta = 1.0f - 0.0001f; // correct_iq.h:23, correct_iq.cpp:9
        flane_walk(x, y, chunk_begin(g, k), chunk_end(g, k), [&](const float v) {
            acc = acc * beta + v * alpha;
            return v - acc;
        });
        endst[k] = DcState{acc, 0.0f};
    }

    __global__ __launch_bounds__(64) void k_fagc(const float *x, float *y, ChunkGeom g, FagcParams p, const AgcState *start0, AgcState *spec, AgcState *endst, const int *redo,
                                                  int nredo)
    {
        const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
        int k;
        float gain;
        const auto step = [&](const float v) {
            const float out = v * gain;
            gain += p.rate * (p.reference - fabsf(out));
            if (p.max_gain > 0.0f && gain > p.max_gain)
                gain = p.max_gain;
            return out;
        };
        if (redo)
        {
            if (idx >= nredo)
                return;
            k = redo[idx];
            gain = spec[k].gain;
        }
        else
        {
            k = idx;
            if (k >= g.K)
                return;
            if (k == 0)
                gain = start0->gain;
            else
            {
                gain = p.init_gain;
                flane_walk(x, nullptr, chunk_begin(g, k) - g.W, chunk_begin(g, k), step);
            }
            spec[k] = AgcState{gain};
        }
        flane_walk(x, y, chunk_begin(g, k), chunk_end(g, k), step);
        endst[k] = AgcState{gain};
    }

    __global__ __launch_bounds__(256) void k_ffir(const float *x, float *y, long long n, const float *__restrict__ rtaps, int ntaps)
    {
        __shared__ float t[FSK_HIST];
        for (int j = (int)threadIdx.x; j < ntaps; j += (int)blockDim.x)
            t[j] = rtaps[j];
        __syncthreads();
        const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n)
            return;
        const float *w = x + i - (ntaps - 1);
        float s = 0.0f;
        for (int j = 0; j < ntaps; j++)
            s += w[j] * t[j];
        y[i] = s;
    }

    // one symbol of MMClockRecoveryBlock<float>::work (clock_recovery_mm.cpp:54-120): the window x[inc - 7 .. inc] against arm rint(mu * 128)
    __device__ __forceinline__ float fmm_iter(FmmState &s, const FmmParams &p, const float *x, const float *bank, const float omega_gain, const float mu_gain)
    {
        int imu = (int)rintf(s.mu * 128.0f);
        if (imu < 0)
            imu = 0;
        if (imu >= 128)
            imu = 127;
        const float *w = x + s.inc - 7, *t = bank + imu * 8;
        float sample = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; j++)
            sample += w[j] * t[j];
        float pe = (s.last < 0 ? -1.0f : 1.0f) * sample - (sample < 0 ? -1.0f : 1.0f) * s.last;
        pe = pe < -1.0f ? -1.0f : (pe > 1.0f ? 1.0f : pe); // branched_clip(phase_error, 1.0)
        s.last = sample;
        s.omega = s.omega + omega_gain * pe;
        float d = s.omega - p.omega_mid;
        d = d < -p.omega_limit ? -p.omega_limit : (d > p.omega_limit ? p.omega_limit : d);
        s.omega = p.omega_mid + d;
        s.mu = (s.mu + s.omega) + mu_gain * pe;
        const float fl = floorf(s.mu);
        s.inc += (long long)(int)fl;
        s.mu = s.mu - fl;
        if (s.inc < 0)
            s.inc = 0;
        return sample;
    }

    // A lane per chunk, the phases of k_mm: warm-up in front of the chunk (nothing stored; spec = the state at the first symbol inside the chunk), the chunk
    // (its symbols into the lane's row; endst = the state at the first symbol behind it), up to two look-ahead symbols behind the chunk end (stored behind
    // the chunk's: what k_mm_verdict hands to the stream when the successor starts a symbol late).
    __global__ __launch_bounds__(64) void k_fmm(const float *x, float *rows, int *counts, ChunkGeom g, FmmParams p, const FmmState *start0, FmmState *spec, FmmState *endst,
                                                 MmCert *spec_c, MmCert *end_c, const int *redo, int nredo)
    {
        __shared__ float bank[128 * 8];
        for (int i = (int)threadIdx.x; i < 128 * 8; i += (int)blockDim.x)
            bank[i] = p.bank[i];
        __syncthreads();
        const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
        int k;
        FmmState s;
        int phase = 1;
        if (redo)
        {
            if (idx >= nredo)
                return;
            k = redo[idx];
            s = spec[k];
        }
        else
        {
            k = idx;
            if (k >= g.K)
                return;
            if (k == 0)
                s = *start0;
            else
            {
                s.mu = p.init_mu;
                s.omega = p.omega_mid;
                s.last = 0.0f;
                s.pad = 0;
                s.inc = chunk_begin(g, k) - g.W;
                phase = 0;
            }
        }
        const long long b = chunk_begin(g, k), e = chunk_end(g, k);
        float *o = rows + (size_t)k * p.cap;
        int cnt = 0, nx = 0, wsym = 0;
        if (!redo && k == 0)
        {
            spec[0] = s;
            spec_c[0] = MmCert{s.mu, s.omega, s.inc};
        }
        // a symbol advances the lane by omega_mid - omega_limit samples or more; a state that does not (a NaN in the input stalls mu for good) must not keep
        // the lane in this loop: past twice the symbols its span can hold, the lane is put behind the stream's end with a fresh loop state
        const long long span = (e > s.inc ? e - s.inc : 0) + 64;
        long long budget = 2 * span + 64;
        for (;;)
        {
            if (--budget < 0)
            {
                s.mu = p.init_mu;
                s.omega = p.omega_mid;
                s.last = 0.0f;
                s.inc = g.n;
            }
            if (phase == 0 && s.inc >= b)
            {
                spec[k] = s;
                spec_c[k] = MmCert{s.mu, s.omega, s.inc};
                phase = 1;
            }
            if (phase == 1 && s.inc >= e)
            {
                counts[2 * k] = cnt;
                endst[k] = s;
                end_c[k] = MmCert{s.mu, s.omega, s.inc};
                phase = 2;
                if (k + 1 >= g.K)
                    break;
            }
            if (phase == 2 && (nx >= 2 || s.inc >= g.n))
                break;
            const bool fast = phase == 0 && wsym < p.fast_syms;
            wsym++;
            const float v = fmm_iter(s, p, x, bank, fast ? 0.0f : p.omega_gain, fast ? p.mu_gain * p.fast_mult : p.mu_gain);
            if (phase != 0)
            {
                if (cnt + nx < p.cap)
                    o[cnt + nx] = v;
                if (phase == 1)
                    cnt++;
                else
                    nx++;
            }
        }
        counts[2 * k + 1] = nx;
    }

    __global__ __launch_bounds__(256) void k_fquant(const float *rows, const int *seg, const long long *offsets, int K, int cap, float scale, int8_t *soft, long long soft_cap,
                                                    float *syms, long long syms_cap)
    {
        const int k = (int)blockIdx.x;
        if (k >= K)
            return;
        const int cnt = seg[2 * k + 1];
        const long long off = offsets[k];
        const float *s = rows + (size_t)k * cap + seg[2 * k];
        for (int j = (int)threadIdx.x; j < cnt; j += (int)blockDim.x)
        {
            const float v = s[j];
            const long long o = off + j;
            if (o < soft_cap)
                soft[o] = sd_clamp8(v * scale);
            if (syms && o < syms_cap)
                syms[o] = v;
        }
    }

    __global__ __launch_bounds__(256) void k_fmean_abs(const float *x, long long n, double *partial)
    {
        __shared__ double acc[256];
        const long long stride = (long long)gridDim.x * blockDim.x;
        double a = 0;
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
            a += fabs((double)x[i]);
        acc[threadIdx.x] = a;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1)
        {
            if ((int)threadIdx.x < s)
                acc[threadIdx.x] += acc[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0)
            partial[blockIdx.x] = acc[0];
    }

    __global__ __launch_bounds__(FSK_HIST) void k_fhist_slide(float *hist, const float *cur, long long ncur)
    {
        const int i = (int)threadIdx.x;
        const long long src = (long long)i + ncur - FSK_HIST; // index into cur; negative: still inside the old history
        const float v = src >= 0 ? cur[src] : hist[FSK_HIST + src];
        __syncthreads();
        hist[i] = v;
    }

    void launch_fquad(const cf32 *x, float *y, long long n, float gain, const float *phase_in, float *phase_out, hipStream_t st)
    {
        if (n <= 0)
            return;
        ProfScope _ps("k_fquad", st);
        hipLaunchKernelGGL(k_fquad, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, y, n, gain, phase_in, phase_out);
    }
    void launch_fdc_partial(const float *x, const ChunkGeom &g, double *partial, hipStream_t st)
    {
        ProfScope _ps("k_fdc_partial", st);
        hipLaunchKernelGGL(k_fdc_partial, dim3(g.K), dim3(256), 0, st, x, g, partial);
    }
    void launch_fdc(const float *x, float *y, const ChunkGeom &g, const DcState *starts, DcState *spec, DcState *endst, const int *redo, int nredo, hipStream_t st)
    {
        const int n = redo ? nredo : g.K;
        if (n <= 0)
            return;
        ProfScope _ps("k_fdc", st);
        hipLaunchKernelGGL(k_fdc, dim3((n + 63) / 64), dim3(64), 0, st, x, y, g, starts, spec, endst, redo, nredo);
    }
    void launch_fagc(const float *x, float *y, const ChunkGeom &g, const FagcParams &p, const AgcState *start0, AgcState *spec, AgcState *endst, const int *redo, int nredo,
                     hipStream_t st)
    {
        const int n = redo ? nredo : g.K;
        if (n <= 0)
            return;
        ProfScope _ps("k_fagc", st);
        hipLaunchKernelGGL(k_fagc, dim3((n + 63) / 64), dim3(64), 0, st, x, y, g, p, start0, spec, endst, redo, nredo);
    }
    void launch_ffir(const float *x, float *y, long long n, const float *rtaps_dev, int ntaps, hipStream_t st)
    {
        if (n <= 0)
            return;
        if (ntaps < 1 || ntaps > FSK_HIST)
            throw HipError("real FIR: tap count outside 1 .. " + std::to_string(FSK_HIST));
        ProfScope _ps("k_ffir", st);
        hipLaunchKernelGGL(k_ffir, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, y, n, rtaps_dev, ntaps);
    }
    void launch_fmm(const float *x, float *rows, int *counts, const ChunkGeom &g, const FmmParams &p, const FmmState *start0, FmmState *spec, FmmState *endst, MmCert *spec_c,
                    MmCert *end_c, const int *redo, int nredo, hipStream_t st)
    {
        const int n = redo ? nredo : g.K;
        if (n <= 0)
            return;
        ProfScope _ps("k_fmm", st);
        hipLaunchKernelGGL(k_fmm, dim3((n + 63) / 64), dim3(64), 0, st, x, rows, counts, g, p, start0, spec, endst, spec_c, end_c, redo, nredo);
    }
    void launch_fquant(const float *rows, const int *seg, const long long *offsets, int K, int cap, float scale, int8_t *soft, long long soft_cap, float *syms,
                       long long syms_cap, hipStream_t st)
    {
        if (K <= 0)
            return;
        ProfScope _ps("k_fquant", st);
        hipLaunchKernelGGL(k_fquant, dim3(K), dim3(256), 0, st, rows, seg, offsets, K, cap, scale, soft, soft_cap, syms, syms_cap);
    }
    void launch_fmean_abs(const float *x, long long n, double *partial, hipStream_t st)
    {
        ProfScope _ps("k_fmean_abs", st);
        hipLaunchKernelGGL(k_fmean_abs, dim3(64), dim3(256), 0, st, x, n, partial);
    }
    void launch_fhist_slide(float *hist, const float *cur, long long ncur, hipStream_t st)
    {
        if (ncur <= 0)
            return;
        hipLaunchKernelGGL(k_fhist_slide, dim3(1), dim3(FSK_HIST), 0, st, hist, cur, ncur);
    }
#endif // SDHIP_FSK_KERNELS_IMPL
} // namespace sdhip
