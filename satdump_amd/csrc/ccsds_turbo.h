// ccsds_turbo.h -- CCSDSTurboDecoderModule::process() (src-core/pipeline/modules/ccsds/module_ccsds_turbo_decoder.cpp:139-257): a BPSK soft stream read in
// buffers of F = A + n (L + 4) bytes (A = 64 / 96 / 128 / 192 ASM bytes, n = 2 / 3 / 4 / 6 code bits per trellis step, L = 8 base information bits) -> the ASM
// correlation at every position of the read -> the module's slide -> derand_ccsds_soft -> CCSDSTurbo::decode (common/codings/turbo/ccsds_turbo.cpp:156-198) over
// turbo_decode / convcode_extrinsic (libs/deepspace-turbo) -> 1A CF FC 1D + base bytes where the CRC-16 holds. Included from lrpt_decoder.hip. gfx950, wave64.
//   k_ct_correlate  thread per stream position: the dot product with the +-1 ASM, soft * (1 / 127) in float, summed left to right from 0 without FMA. A position's
//                   answer does not depend on the read it falls in, so it is computed once per position (256 positions + an A - 1 halo in LDS per block)
//   k_ct_spec       workgroup per grid read behind an origin: the read's decision, the arg-max of |c| over its F - A positions (strict >, so the first position)
//   k_ct_walk       follows the answers while they say 0, takes the first slide as a new origin (k_cl_walk's bookkeeping with a slide that moves the origin by F + pos)
//   k_ct_chain      the serial walk for a stream that keeps sliding
//   k_ct_recur      convcode_extrinsic's two recursions (libconvcodes.c:380-467): 16 lanes own one frame, a state per lane, four frames per wave; blockIdx.y picks the
//                   backward or the forward recursion, which do not depend on each other. The previous column lives in LDS (128 bytes a frame, double buffered);
//                   next_state / neighbors are table look-ups into it; the column maximum is taken by every lane over the 16 raw values. The module's buffer rule,
//                   the derandomiser, the float conversion, the sign, the depuncturing and the split into the two constituent streams are fused into the load (ct_rho)
//   k_ct_ext        the extrinsic step (libconvcodes.c:476-509), thread per (frame, trellis step): the two 16-term folds over the states in the reference's order,
//                   the a-priori arrays rewritten in place (through the interleaver for the lower code, so no message is ever moved), the decision on the last pass
//   k_ct_pack       decisions -> bytes MSB first, CRC-16 (0x1021 from 0xFFFF) over base - 2 bytes against the last two
//   k_ct_emit       the frames whose CRC holds, in order, behind 1A CF FC 1D
// exp_sum(a, b) = (a > b) ? a : b + log(1 + exp(-|a - b|)) is neither commutative nor associative: every fold runs in the reference's order, every sum keeps its
// association, squares are x * x, all in double. Where exp(-|a - b|) < 2^-53 the reference adds log(1.0) = 0: that is what is added here, without the two calls.
// Both recursions are stored (2 x 16 x (L + 4) doubles a frame): the extrinsic step then is parallel over the trellis steps instead of the serial tail of each one.
// Kept quirks: the slide moves `pos` bytes, not F - pos (B[i] below: a slide of pos <= F / 2 decodes a buffer whose middle is stale); the derandomiser is ~x; the
// PN sequence restarts at the codeword; sigma^2 is the float product 0.707f * 0.707f. Not emulated: the module's last iteration at the end of a file, which decodes
// the previous buffer once more after derandomising it twice.
#pragma once
#include "../../include/sdhip.h"
#include "common.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <vector>

namespace sdhip
{
    constexpr int CT_MAX_ASM = 192;
    constexpr int CT_READS = 4096;                       // reads per internal round of a call (bounds the correlation table)
    constexpr size_t CT_SCRATCH = (size_t)24 << 30;      // bytes of recursion columns a decoder piece may hold (4096 frames of base 1115 take 9.4 GB)
    constexpr double CT_THRESHOLD = 1e10;                // convcode_extrinsic's `threshold`

    struct CtGeom
    {
        int rate, base;
        int L, steps; // information bits, trellis steps (L + 4)
        int A, F;     // ASM soft bytes, soft bytes per read
        int nu, nl;   // components of the upper / lower code
        int wire;     // code bits per trellis step on the wire (2 / 3 / 4 / 6)
    };
    struct CtAsm
    {
        float w[CT_MAX_ASM];
    };
    struct CtTables
    {
        unsigned char next[16][2];   // next_state[s][u]
        unsigned char prev[16][2];   // neighbors[s][n]: state | input << 4
        unsigned char out[2][16][2]; // output[s][u] of the upper / lower code, bit j = component j
    };
    struct CtSpec
    {
        int pos, swapped;
        float cor;
    };
    struct CtDesc
    {
        long long origin; // where the read started in the stream handed to the chain
        int pos, swapped;
        float cor;
    };
    struct CtIn
    {
        int mode;            // 0: the stream, frames named by descriptors | 1: float codewords as CCSDSTurbo::decode receives them | 2: one constituent code's double stream
        const int8_t *soft;  // mode 0
        const CtDesc *descs; // mode 0
        const float *cw;     // mode 1, `stride` floats a frame
        const double *cs;    // mode 2, `stride` doubles a frame
        int stride;
        unsigned pn[8];      // ccsds_soft_pn, a bit per entry
    };

    __global__ __launch_bounds__(256) void k_ct_correlate(const int8_t *__restrict__ soft, long long n, CtAsm sw, int A, float *__restrict__ cor)
    {
        __shared__ float conv[256 + CT_MAX_ASM];
        const int tid = (int)threadIdx.x;
        const long long base = (long long)blockIdx.x * 256;
        for (int i = tid; i < 256 + A - 1; i += 256)
        {
            const long long j = base + i;
            conv[i] = j < n ? (float)soft[j] * (1.0f / 127.0f) : 0.0f; // volk_8i_s32f_convert_32f(.., 127, ..)
        }
        __syncthreads();
        const long long p = base + tid;
        if (p + A > n)
            return;
        float acc = 0.0f;
        for (int x = 0; x < A; x++)
            acc = acc + conv[tid + x] * sw.w[x]; // (-ffp-contract=off: multiply, then add)
        cor[p] = acc;
    }

    // |c| first, the lowest position among equals; 0 = neither `c > best` nor `-c > best` ever held
    __device__ __forceinline__ unsigned long long ct_key(float c, int p)
    {
        const float a = c < 0.0f ? -c : c;
        return a > 0.0f ? ((unsigned long long)__float_as_uint(a) << 32) | (unsigned)(0x7FFFFFFF - p) : 0ull;
    }
    // one read at o over the per-position answers: `if (c > best) ..; if (-c > best) ..` for pos < F - A
    template <int NT>
    __device__ __forceinline__ CtSpec ct_read_decision(const float *__restrict__ cor, long long o, int npos, unsigned long long *red)
    {
        unsigned long long best = 0;
        for (int p = (int)threadIdx.x; p < npos; p += NT)
        {
            const unsigned long long k = ct_key(cor[o + p], p);
            best = best > k ? best : k;
        }
        best = cl_block_max<NT>(best, red);
        if (best == 0)
            return CtSpec{0, 0, 0.0f};
        const int pos = 0x7FFFFFFF - (int)(unsigned)(best & 0xFFFFFFFFull);
        return CtSpec{pos, cor[o + pos] < 0.0f ? 1 : 0, __uint_as_float((unsigned)(best >> 32))};
    }
    __global__ __launch_bounds__(256) void k_ct_spec(const float *__restrict__ cor, long long origin, int F, int A, CtSpec *spec, int nreads)
    {
        __shared__ unsigned long long red[256];
        const int k = (int)blockIdx.x;
        if (k >= nreads)
            return;
        const CtSpec s = ct_read_decision<256>(cor, origin + (long long)k * F, F - A, red);
        if (threadIdx.x == 0)
            spec[k] = s;
    }
    // state[0] = reads so far, state[1] = 1 when the stream is used up (or the slide's extra read is not complete yet), consumed = where the chain stands
    __global__ __launch_bounds__(1024) void k_ct_walk(const CtSpec *__restrict__ spec, int nreads, long long n, long long origin, int F, CtDesc *descs, int max_frames,
                                                       int *state, long long *consumed, CtSpec *pend)
    {
        __shared__ int s_first;
        const int tid = (int)threadIdx.x;
        const int cnt0 = state[0];
        const long long fit = (n - origin) / F;
        int limit = nreads;
        if (fit < (long long)limit)
            limit = (int)(fit < 0 ? 0 : fit);
        if (max_frames - cnt0 < limit)
            limit = max_frames - cnt0 < 0 ? 0 : max_frames - cnt0;
        if (tid == 0)
            s_first = limit;
        __syncthreads();
        for (int k = tid; k < limit; k += 1024)
            if (spec[k].pos != 0)
                atomicMin(&s_first, k);
        __syncthreads();
        const int first = s_first;
        for (int k = tid; k < first; k += 1024)
            descs[cnt0 + k] = CtDesc{origin + (long long)k * F, 0, spec[k].swapped, spec[k].cor};
        if (tid == 0)
        {
            int cnt = cnt0 + first, done = 1;
            long long o = origin + (long long)first * F;
            if (first < limit)
            { // the first slide: `pos` more bytes are read behind the buffer; the next read starts behind them
                const CtSpec sp = spec[first];
                if (o + F + sp.pos <= n)
                {
                    descs[cnt] = CtDesc{o, sp.pos, sp.swapped, sp.cor};
                    cnt++;
                    o += (long long)F + sp.pos;
                    done = (o + F <= n && cnt < max_frames) ? 0 : 1;
                }
                else
                    *pend = sp; // the extra read is not complete yet -- the read stays for the next call; the module has its correlation already
            }
            state[0] = cnt;
            state[1] = done;
            *consumed = o;
        }
    }
    __global__ __launch_bounds__(1024) void k_ct_chain(const float *__restrict__ cor, long long n, long long o0, int F, int A, CtDesc *descs, int max_frames, int *count,
                                                        long long *consumed, CtSpec *pend)
    {
        __shared__ unsigned long long red[1024];
        long long o = o0;
        int cnt = 0;
        while (o + F <= n && cnt < max_frames)
        {
            const CtSpec s = ct_read_decision<1024>(cor, o, F - A, red);
            if (s.pos != 0 && o + F + s.pos > n)
            {
                if (threadIdx.x == 0)
                    *pend = s;
                break;
            }
            if (threadIdx.x == 0)
                descs[cnt] = CtDesc{o, s.pos, s.swapped, s.cor};
            cnt++;
            o += (long long)F + s.pos;
        }
        if (threadIdx.x == 0)
        {
            *count = cnt;
            *consumed = o;
        }
    }

    // ---- the decoder --------------------------------------------------------------------------------------------------------------------------------------
    // received[components * i + j] of constituent code `code` for frame f: what turbo_decode's serial-to-parallel split (libturbocodes.c:149-158) hands
    // convcode_extrinsic, from the bytes the module decodes. The buffer after the slide, with o the read's origin and S the stream: B[i] = S[o + pos + i] for
    // i < pos or i >= F - pos, S[o + i] otherwise (memmove(buf, buf + pos, pos), then pos bytes read into buf[F - pos ..]).
    struct CtFrame
    { // what ct_rho needs of one frame, fetched once
        const int8_t *soft; // the stream at the read's origin
        int pos, swapped;
    };
    __device__ __forceinline__ CtFrame ct_frame(const CtIn &in, int f)
    {
        if (in.mode != 0)
            return CtFrame{nullptr, 0, 0};
        const CtDesc d = in.descs[f];
        return CtFrame{in.soft + d.origin, d.pos, d.swapped};
    }
    __device__ __forceinline__ double ct_rho(const CtIn &in, const CtGeom &g, const CtFrame &fr, int f, int code, int i, int j)
    {
        if (in.mode == 2)
            return in.cs[(size_t)f * in.stride + (size_t)i * (code ? g.nl : g.nu) + j];
        const int r = code ? g.nu + j : j; // place inside the trellis step of the serial stream
        int w;
        if (g.rate == SDHIP_CCSDS_TURBO_RATE_1_2)
        { // depunctured to the rate 1/3 layout: puncturing(k) keeps 0, drops 2 in even blocks and 1 in odd ones
            if (r != 0 && ((i & 1) ? r == 1 : r == 2))
                return 0.0;
            w = 2 * i + (r ? 1 : 0);
        }
        else
            w = i * g.wire + r;
        if (in.mode == 1)
            return (double)in.cw[(size_t)f * in.stride + w];
        const int b = g.A + w;
        int v = (int)fr.soft[b + ((b < fr.pos || b >= g.F - fr.pos) ? fr.pos : 0)];
        const int k = w % 255;
        if ((in.pn[k >> 5] >> (k & 31)) & 1u)
            v = (int)(signed char)~v; // ~x on an int8
        const float x = (float)v * (1.0f / 127.0f);
        return (double)(fr.swapped ? -x : x);
    }
    __device__ __forceinline__ double ct_exp_sum(double a, double b)
    {
        const double diff = a - b;
        if (a > b)
            return a;
        const double d = -diff > 0 ? diff : -diff;
        if (d < -40.0)
            return b + 0.0; // exp(d) < 2^-53: 1 + exp(d) == 1 and log(1) == 0
        return b + log(1 + exp(d));
    }
    // -g / (2 sigma^2) of one trellis branch: g = sum over the components of (rho_j - (2 out_j - 1))^2, from 0, in order
    __device__ __forceinline__ double ct_gamma(const double *rho, int nc, unsigned o, double nv2)
    {
        double g = 0;
        for (int j = 0; j < nc; j++)
        {
            const double x = rho[j] - (double)(2 * (int)((o >> j) & 1u) - 1);
            g = g + x * x;
        }
        return -g / nv2;
    }
    __device__ __forceinline__ double ct_app(const double *__restrict__ msgs, const int *__restrict__ pi, int L, int u, int i, double log_half)
    { // app[u][i]: the a-priori array as the constituent code sees it (the lower code reads through the interleaver), log(0.5) over the tail
        return i < L ? msgs[(size_t)u * L + (pi ? pi[i] : i)] : log_half;
    }

    // cols: [frame][dir][step][16], dir 0 = backward, 1 = forward; msgs: [frame][2][L]
    __global__ __launch_bounds__(64) void k_ct_recur(CtIn in, CtGeom g, CtTables t, int code, int f0, int nframes, const double *__restrict__ msgs, const int *__restrict__ pi,
                                                      double *__restrict__ cols, double nv2, double log_half)
    {
        __shared__ double col[2][4][16];
        const int tid = (int)threadIdx.x, q = tid >> 4, s = tid & 15, dir = (int)blockIdx.y;
        int f = (int)blockIdx.x * 4 + q;
        const bool live = f < nframes;
        if (!live)
            f = nframes - 1; // (the barriers below are the workgroup's)
        const int nc = code ? g.nl : g.nu, steps = g.steps;
        const double *m = msgs + (size_t)f * 2 * g.L;
        double *c = cols + ((size_t)f * 2 + dir) * steps * 16;
        const CtFrame fr = ct_frame(in, f0 + f);
        double rho[4] = {0.0, 0.0, 0.0, 0.0}, app[2], nrho[4] = {0.0, 0.0, 0.0, 0.0}, napp[2] = {0.0, 0.0};
        double mx = 0.0; // what the raw column in LDS still has to lose
        int cur = 0;
        const double init = s == 0 ? 0.0 : -CT_THRESHOLD;
        col[0][q][s] = init;
        if (live)
            c[(size_t)(dir ? 0 : steps - 1) * 16 + s] = init;
        auto fetch = [&](int k, double *r, double *a) { // the symbols and a-priori values that enter step k of the walk: those of trellis step `src`
            const int src = dir ? k - 1 : steps - k;
            for (int j = 0; j < nc; j++)
                r[j] = ct_rho(in, g, fr, f0 + f, code, src, j);
            a[0] = ct_app(m, pi, g.L, 0, src, log_half);
            a[1] = ct_app(m, pi, g.L, 1, src, log_half);
        };
        fetch(1, rho, app);
        __syncthreads();
        for (int k = 1; k < steps; k++)
        {
            const int i = dir ? k : steps - 1 - k; // the column written
            if (k + 1 < steps)
                fetch(k + 1, nrho, napp); // (none of it depends on the recursion: in flight under this step's exp / log)
            double acc = -CT_THRESHOLD;
            for (int n = 0; n < 2; n++)
            {
                int other, u;
                unsigned o;
                if (dir)
                { // neighbors[s][n]: the predecessor and its input
                    other = t.prev[s][n] & 15;
                    u = t.prev[s][n] >> 4;
                    o = t.out[code][other][u];
                }
                else
                {
                    u = n;
                    other = t.next[s][u];
                    o = t.out[code][s][u];
                }
                const double term = app[u] + (col[cur][q][other] - mx) + ct_gamma(rho, nc, o, nv2);
                acc = ct_exp_sum(acc, term);
            }
            cur ^= 1;
            col[cur][q][s] = acc;
            __syncthreads();
            double top = col[cur][q][0];
            for (int x = 0; x < 16; x++)
                top = col[cur][q][x] > top ? col[cur][q][x] : top;
            mx = top;
            if (live)
                c[(size_t)i * 16 + s] = acc - mx;
            for (int j = 0; j < 4; j++)
                rho[j] = nrho[j];
            app[0] = napp[0];
            app[1] = napp[1];
        }
    }

    __global__ __launch_bounds__(256) void k_ct_ext(CtIn in, CtGeom g, CtTables t, int code, int f0, int nframes, double *__restrict__ msgs, const int *__restrict__ pi,
                                                     const double *__restrict__ cols, double nv2, int decide, unsigned char *__restrict__ bits)
    {
        const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
        if (id >= (long long)nframes * g.L)
            return;
        const int f = (int)(id / g.L), i = (int)(id % g.L);
        const int nc = code ? g.nl : g.nu;
        const double *bw = cols + ((size_t)f * 2 + 0) * g.steps * 16 + (size_t)i * 16;
        const double *fw = cols + ((size_t)f * 2 + 1) * g.steps * 16 + (size_t)i * 16;
        double rho[4], b[16];
        const CtFrame fr = ct_frame(in, f0 + f);
        for (int j = 0; j < nc; j++)
            rho[j] = ct_rho(in, g, fr, f0 + f, code, i, j);
        for (int s = 0; s < 16; s++)
            b[s] = bw[s];
        double e[2];
        for (int u = 0; u < 2; u++)
        {
            double acc = -CT_THRESHOLD;
            for (int s = 0; s < 16; s++)
                acc = ct_exp_sum(acc, fw[s] + b[t.next[s][u]] + ct_gamma(rho, nc, t.out[code][s][u], nv2));
            e[u] = acc;
        }
        const int k = pi ? pi[i] : i;
        double *m = msgs + (size_t)f * 2 * g.L;
        if (decide)
        { // `one > zero` on the a-priori values the pass received; turbo_deinterleave puts decision i at d_pi[i]
            const double one = m[(size_t)g.L + k] + e[1], zero = m[k] + e[0];
            bits[(size_t)(f0 + f) * g.L + k] = one > zero ? 1 : 0;
        }
        m[k] = e[0];
        m[(size_t)g.L + k] = e[1];
    }
    __global__ __launch_bounds__(256) void k_ct_fill(double *p, size_t n, double v)
    {
        const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
        if (i < n)
            p[i] = v;
    }
    // bits [frame][L] -> frames [frame][base], ok[frame] = the CRC holds
    __global__ __launch_bounds__(256) void k_ct_pack(const unsigned char *__restrict__ bits, int base, unsigned char *__restrict__ frames, int *__restrict__ ok)
    {
        const int f = (int)blockIdx.x;
        const unsigned char *b = bits + (size_t)f * base * 8;
        unsigned char *o = frames + (size_t)f * base;
        for (int k = (int)threadIdx.x; k < base; k += 256)
        {
            unsigned v = 0;
            for (int x = 0; x < 8; x++)
                v = (v << 1) | (b[k * 8 + x] & 1u);
            o[k] = (unsigned char)v;
        }
        __syncthreads();
        if (threadIdx.x == 0)
        { // GenericCRC(16, 0x1021, 0xFFFF, 0x0, false, false)
            unsigned crc = 0xFFFFu;
            for (int k = 0; k < base - 2; k++)
            {
                crc ^= (unsigned)o[k] << 8;
                for (int x = 0; x < 8; x++)
                    crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x1021u) & 0xFFFFu : (crc << 1) & 0xFFFFu;
            }
            ok[f] = crc == (((unsigned)o[base - 2] << 8) | o[base - 1]) ? 1 : 0;
        }
    }
    __global__ __launch_bounds__(256) void k_ct_emit(const unsigned char *__restrict__ frames, const int *__restrict__ sel, int base, unsigned char *__restrict__ out)
    {
        const unsigned char *src = frames + (size_t)sel[blockIdx.x] * base;
        unsigned char *o = out + (size_t)blockIdx.x * (base + 4);
        for (int k = (int)threadIdx.x; k < base + 4; k += 256)
            o[k] = k >= 4 ? src[k - 4] : (unsigned char)(k == 0 ? 0x1Au : (k == 1 ? 0xCFu : (k == 2 ? 0xFCu : 0x1Du)));
    }

    // ---- host ------------------------------------------------------------------------------------------------------------------------------------------------
    inline bool ct_geometry(int rate, int base, CtGeom &g)
    {
        static const int A[4] = {64, 96, 128, 192}, wire[4] = {2, 3, 4, 6}, nu[4] = {2, 2, 3, 4}, nl[4] = {1, 1, 1, 2};
        if (rate < 0 || rate > 3 || !(base == 223 || base == 446 || base == 892 || base == 1115))
            return false;
        g.rate = rate;
        g.base = base;
        g.L = base * 8;
        g.steps = g.L + 4;
        g.A = A[rate];
        g.wire = wire[rate];
        g.F = g.A + g.wire * g.steps;
        g.nu = nu[rate];
        g.nl = nl[rate];
        return true;
    }
    // The attached sync markers of CCSDS 131.0-B section 9.3.5: 0x034776C7272895B0 (rate 1/2), 0x25D5C0CE8990F6C9461BF79C (1/3),
    // 0x034776C7272895B0FCB88938D8D76A4F (1/4), 0x25D5C0CE8990F6C9461BF79CDA2A3F31766F0936B9E40863 (1/6); a one is +1, a zero -1
    inline CtAsm ct_asm(int rate)
    {
        static const unsigned char m12[] = {0x03, 0x47, 0x76, 0xC7, 0x27, 0x28, 0x95, 0xB0, 0xFC, 0xB8, 0x89, 0x38, 0xD8, 0xD7, 0x6A, 0x4F};
        static const unsigned char m13[] = {0x25, 0xD5, 0xC0, 0xCE, 0x89, 0x90, 0xF6, 0xC9, 0x46, 0x1B, 0xF7, 0x9C, 0xDA, 0x2A, 0x3F, 0x31, 0x76, 0x6F, 0x09, 0x36, 0xB9, 0xE4, 0x08, 0x63};
        const unsigned char *m = (rate == SDHIP_CCSDS_TURBO_RATE_1_2 || rate == SDHIP_CCSDS_TURBO_RATE_1_4) ? m12 : m13; // the short markers are the long ones' first halves
        CtGeom g;
        ct_geometry(rate, 223, g);
        CtAsm a;
        memset(&a, 0, sizeof(a));
        for (int i = 0; i < g.A; i++)
            a.w[i] = ((m[i >> 3] >> (7 - (i & 7))) & 1) ? 1.0f : -1.0f;
        return a;
    }
    // The interleaver of CCSDS 131.0-B section 6.3 (k1 = 8, k2 = base, p = 31 37 43 47 53 59 61 67), 0-based: out[s - 1] = pi(s) - 1
    inline void ct_interleaver(int base, int *out)
    {
        static const int p[8] = {31, 37, 43, 47, 53, 59, 61, 67};
        const int k1 = 8, k2 = base;
        for (int s = 1; s <= k1 * k2; s++)
        {
            const int m = (s - 1) % 2;
            const int i = (s - 1) / (2 * k2);
            const int j = (s - 1) / 2 - i * k2;
            const int t = (19 * i + 1) % (k1 / 2);
            const int q = t % 8 + 1;
            const int c = (p[q - 1] * j + 21 * m) % k2;
            out[s - 1] = 2 * (t + c * (k1 / 2) + 1) - m - 1;
        }
    }
    // The 16-state constituent encoder of CCSDS 131.0-B section 6.3: feedback G0 = 10011, forward G1 = 11011, G2 = 10101, G3 = 11111. The state holds the four
    // register cells, the newest in bit 3. The cell fed back is input + (taps 3 and 4 of G0); an output is its polynomial over (that cell, the four old cells), and
    // G0's own output is the input bit. Upper code: G0 G1 | G0 G1 | G0 G2 G3 | G0 G1 G2 G3 for rates 1/2 1/3 1/4 1/6; lower code: G1 | G1 | G1 | G1 G3.
    // prev[s] lists the (state, input) pairs that lead to s in the order state 0 .. 15, input 0 before 1 -- the order the forward fold takes them in.
    inline CtTables ct_tables(int rate)
    {
        static const int G[4] = {0x13, 0x1B, 0x15, 0x1F};
        static const int upper[4][4] = {{0, 1, -1, -1}, {0, 1, -1, -1}, {0, 2, 3, -1}, {0, 1, 2, 3}}, lower[4][2] = {{1, -1}, {1, -1}, {1, -1}, {1, 3}};
        CtTables t;
        memset(&t, 0, sizeof(t));
        int filled[16] = {0};
        for (int s = 0; s < 16; s++)
            for (int u = 0; u < 2; u++)
            {
                const int fb = (((s >> 1) ^ s) & 1) ^ u; // cells 3 and 4 (bits 1 and 0) + the input
                const int ns = (s >> 1) | (fb << 3);
                t.next[s][u] = (unsigned char)ns;
                t.prev[ns][filled[ns]++] = (unsigned char)(s | (u << 4));
                auto output = [&](int poly) { // bit 4 of the polynomial meets the new cell, bits 3 .. 0 the old cells newest first
                    int o = ((poly >> 4) & 1) & fb;
                    for (int k = 0; k < 4; k++)
                        o ^= ((poly >> (3 - k)) & 1) & ((s >> (3 - k)) & 1);
                    return o;
                };
                for (int j = 0; j < 4; j++)
                    if (upper[rate][j] >= 0)
                        t.out[0][s][u] |= (unsigned char)(output(G[upper[rate][j]]) << j);
                for (int j = 0; j < 2; j++)
                    if (lower[rate][j] >= 0)
                        t.out[1][s][u] |= (unsigned char)(output(G[lower[rate][j]]) << j);
            }
        return t;
    }

    // turbo_decode (libturbocodes.c:137-201) for frames named by `in`: the iterations over both constituent codes, decisions to d_bits [frame][L]
    struct CtDecoder
    {
        CtGeom g;
        CtTables tab;
        DevBuf<int> d_pi;
        DevBuf<double> d_cols, d_msgs;
        double nv2, log_half;
        int piece; // frames whose columns fit CT_SCRATCH

        CtDecoder(int rate, int base)
        {
            if (!ct_geometry(rate, base, g))
                throw HipError("ccsds_turbo: turbo_rate must be 1/2, 1/3, 1/4 or 1/6 and turbo_base 223, 446, 892 or 1115");
            tab = ct_tables(rate);
            std::vector<int> pi(g.L);
            ct_interleaver(base, pi.data());
            d_pi.reserve(pi.size());
            SD_HIP(hipMemcpy(d_pi.p, pi.data(), pi.size() * sizeof(int), hipMemcpyHostToDevice));
            const float sigma = 0.707; // d_sigma, squared in float at the call site
            nv2 = 2 * (double)(sigma * sigma);
            log_half = log(0.5);
            piece = (int)std::max<size_t>(1, CT_SCRATCH / ((size_t)2 * 16 * g.steps * sizeof(double)));
        }
        void bcjr(const CtIn &in, int code, int f0, int n, const int *pi, int decide, unsigned char *d_bits)
        {
            {
                ProfScope _ps("k_ct_recur", nullptr);
                hipLaunchKernelGGL(k_ct_recur, dim3((unsigned)((n + 3) / 4), 2), dim3(64), 0, nullptr, in, g, tab, code, f0, n, d_msgs.p, pi, d_cols.p, nv2, log_half);
            }
            ProfScope _ps("k_ct_ext", nullptr);
            hipLaunchKernelGGL(k_ct_ext, dim3((unsigned)(((size_t)n * g.L + 255) / 256)), dim3(256), 0, nullptr, in, g, tab, code, f0, n, d_msgs.p, pi, d_cols.p, nv2, decide, d_bits);
        }
        void scratch(int n)
        {
            d_cols.reserve((size_t)n * 2 * 16 * g.steps);
            d_msgs.reserve((size_t)n * 2 * g.L);
        }
        void decode(const CtIn &in, int nframes, int iterations, unsigned char *d_bits)
        {
            if (nframes <= 0)
                return;
            const int npieces = (nframes + piece - 1) / piece, per = (nframes + npieces - 1) / npieces;
            scratch(per);
            for (int f0 = 0; f0 < nframes; f0 += per)
            {
                const int n = std::min(per, nframes - f0);
                const size_t nm = (size_t)n * 2 * g.L;
                hipLaunchKernelGGL(k_ct_fill, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, nullptr, d_msgs.p, nm, log_half);
                for (int it = 0; it < iterations; it++)
                {
                    bcjr(in, 0, f0, n, nullptr, 0, d_bits);
                    bcjr(in, 1, f0, n, d_pi.p, it == iterations - 1 ? 1 : 0, d_bits);
                }
            }
        }
    };

    struct CcsdsTurbo
    {
        sdhip_ccsds_turbo_cfg cfg;
        sdhip_ccsds_turbo_stats stats{};
        CtDecoder dec;
        CtAsm sync;
        CtIn in{};
        int frame_bytes;
        DevBuf<int8_t> stream;
        size_t carry = 0;
        uint64_t stream_base = 0; // stream position of stream[0]
        DevBuf<float> d_cor;
        DevBuf<CtDesc> d_desc;
        DevBuf<CtSpec> d_spec, d_pend;
        DevBuf<int> d_state, d_cnt, d_ok, d_sel;
        DevBuf<long long> d_consumed;
        DevBuf<unsigned char> d_bits, d_frames;
        std::vector<sdhip_ccsds_turbo_desc> descs; // of the last call
        std::deque<std::vector<unsigned char>> outq;

        static const sdhip_ccsds_turbo_cfg &checked(const sdhip_ccsds_turbo_cfg &c)
        {
            CtGeom g;
            if (c.rate < 0 || c.rate > 3)
                throw HipError("Invalid Turbo Rate!");
            if (!ct_geometry(c.rate, c.base, g))
                throw HipError("Turbo Base must be 223, 446, 892 or 1115!");
            if (c.iterations < 1)
                throw HipError("ccsds_turbo: turbo_iters must be at least 1");
            return c;
        }
        explicit CcsdsTurbo(const sdhip_ccsds_turbo_cfg &c) : cfg(checked(c)), dec(((void)hipSetDevice(c.device), c.rate), c.base)
        {
            sync = ct_asm(cfg.rate);
            in.mode = 0;
            cl_soft_pn(in.pn);
            frame_bytes = cfg.base + 4;
            d_state.reserve(2);
            d_cnt.reserve(1);
            d_consumed.reserve(1);
        }

        // the module's loop over the bytes at hand: a descriptor for every read whose bytes are all there, *consumed = where the next read starts
        int chain(const int8_t *base, long long total, long long *consumed_out, CtSpec *pending_read)
        {
            const int F = dec.g.F, A = dec.g.A;
            d_pend.reserve(1);
            SD_HIP(hipMemsetAsync(d_pend.p, 0, sizeof(CtSpec), nullptr)); // pos 0: no read waits for its slide
            d_cor.reserve((size_t)total);
            {
                ProfScope _ps("k_ct_correlate", nullptr);
                const long long npos = total - A + 1;
                hipLaunchKernelGGL(k_ct_correlate, dim3((unsigned)((npos + 255) / 256)), dim3(256), 0, nullptr, base, total, sync, A, d_cor.p);
            }
            const int max_frames = (int)(total / F) + 1;
            d_desc.reserve(max_frames);
            d_spec.reserve(max_frames);
            int nf = 0;
            long long consumed = 0;
            bool chained = false;
            {
                ProfScope _ps("k_ct_spec + k_ct_walk", nullptr);
                SD_HIP(hipMemsetAsync(d_state.p, 0, 2 * sizeof(int), nullptr));
                long long origin = 0;
                int st[2] = {0, 0};
                for (int round = 0; round < 6; round++)
                {
                    const int nreads = (int)((total - origin) / F);
                    if (nreads <= 0)
                    {
                        st[1] = 1;
                        consumed = origin;
                        break;
                    }
                    hipLaunchKernelGGL(k_ct_spec, dim3((unsigned)nreads), dim3(256), 0, nullptr, d_cor.p, origin, F, A, d_spec.p, nreads);
                    hipLaunchKernelGGL(k_ct_walk, dim3(1), dim3(1024), 0, nullptr, d_spec.p, nreads, total, origin, F, d_desc.p, max_frames, d_state.p, d_consumed.p, d_pend.p);
                    SD_HIP(hipMemcpy(st, d_state.p, sizeof(st), hipMemcpyDeviceToHost));
                    SD_HIP(hipMemcpy(&consumed, d_consumed.p, sizeof(long long), hipMemcpyDeviceToHost));
                    origin = consumed;
                    stats.chain_rounds++;
                    if (st[1])
                        break;
                }
                nf = st[0];
                chained = st[1] != 0;
            }
            if (!chained)
            { // a stream that keeps sliding: the serial walk over what is left, behind the reads found so far
                ProfScope _ps("k_ct_chain", nullptr);
                int rest = 0;
                hipLaunchKernelGGL(k_ct_chain, dim3(1), dim3(1024), 0, nullptr, d_cor.p, total, consumed, F, A, d_desc.p + nf, max_frames - nf, d_cnt.p, d_consumed.p, d_pend.p);
                SD_HIP(hipMemcpy(&rest, d_cnt.p, sizeof(int), hipMemcpyDeviceToHost));
                SD_HIP(hipMemcpy(&consumed, d_consumed.p, sizeof(long long), hipMemcpyDeviceToHost));
                nf += rest;
                stats.chain_serial++;
            }
            SD_HIP(hipMemcpy(pending_read, d_pend.p, sizeof(CtSpec), hipMemcpyDeviceToHost));
            *consumed_out = consumed;
            return nf;
        }

        // n more soft bytes (device, at most CT_READS reads' worth); frames to d_out (room for cap_frames). Returns the frames written.
        int64_t piece(const int8_t *d_in, size_t n, unsigned char *d_out, size_t cap_frames)
        {
            const int F = dec.g.F, base_bytes = cfg.base;
            stats.soft_in += n;
            const size_t total = carry + n;
            const int8_t *base = d_in;
            if (carry || total < (size_t)F)
            {
                if (total + 64 > stream.cap)
                {
                    DevBuf<int8_t> bigger;
                    bigger.reserve(total + total / 2 + 64);
                    if (carry)
                        SD_HIP(hipMemcpy(bigger.p, stream.p, carry, hipMemcpyDeviceToDevice));
                    stream.swap(bigger);
                }
                if (n)
                    SD_HIP(hipMemcpy(stream.p + carry, d_in, n, hipMemcpyDeviceToDevice));
                base = stream.p;
            }
            if (total < (size_t)F)
            {
                carry = total;
                return 0;
            }
            long long consumed = 0;
            CtSpec pending_read{0, 0, 0.0f};
            const int nf = chain(base, (long long)total, &consumed, &pending_read);
            int64_t written = 0;
            if (nf > 0)
            {
                d_bits.reserve((size_t)nf * dec.g.L);
                d_frames.reserve((size_t)nf * base_bytes);
                d_ok.reserve(nf);
                d_sel.reserve(nf);
                in.soft = base;
                in.descs = d_desc.p;
                dec.decode(in, nf, cfg.iterations, d_bits.p);
                {
                    ProfScope _ps("k_ct_pack", nullptr);
                    hipLaunchKernelGGL(k_ct_pack, dim3((unsigned)nf), dim3(256), 0, nullptr, d_bits.p, base_bytes, d_frames.p, d_ok.p);
                }
                std::vector<CtDesc> hd(nf);
                std::vector<int> ok(nf), sel;
                SD_HIP(hipMemcpy(hd.data(), d_desc.p, (size_t)nf * sizeof(CtDesc), hipMemcpyDeviceToHost));
                SD_HIP(hipMemcpy(ok.data(), d_ok.p, (size_t)nf * sizeof(int), hipMemcpyDeviceToHost));
                for (int f = 0; f < nf; f++)
                {
                    descs.push_back(sdhip_ccsds_turbo_desc{stream_base + (uint64_t)hd[f].origin, hd[f].pos, hd[f].swapped, hd[f].cor, ok[f]});
                    if (ok[f])
                        sel.push_back(f);
                }
                if (sel.size() > cap_frames)
                    throw HipError("ccsds_turbo: frame output buffer too small");
                if (!sel.empty())
                {
                    ProfScope _ps("k_ct_emit", nullptr);
                    SD_HIP(hipMemcpy(d_sel.p, sel.data(), sel.size() * sizeof(int), hipMemcpyHostToDevice));
                    hipLaunchKernelGGL(k_ct_emit, dim3((unsigned)sel.size()), dim3(256), 0, nullptr, d_frames.p, d_sel.p, base_bytes, d_out);
                }
                written = (int64_t)sel.size();
                stats.reads += nf;
                stats.frames_out += written;
                stats.locked = hd[nf - 1].pos == 0 ? 1 : 0;
                stats.cor = hd[nf - 1].cor;
                stats.crc_lock = ok[nf - 1];
            }
            if (pending_read.pos != 0)
            { // a read whose extra bytes are not there yet: the module has set these before it asks for them (module_ccsds_turbo_decoder.cpp:205-206)
                stats.locked = 0;
                stats.cor = pending_read.cor;
            }
            SD_HIP(hipDeviceSynchronize()); // (the kernels above read `base`, which the copies below may overwrite)
            const size_t rest = total - (size_t)consumed;
            if (rest && (consumed || base != stream.p))
            {
                if (base == stream.p)
                {
                    DevBuf<int8_t> tmp;
                    tmp.reserve(rest);
                    SD_HIP(hipMemcpy(tmp.p, stream.p + consumed, rest, hipMemcpyDeviceToDevice));
                    SD_HIP(hipMemcpy(stream.p, tmp.p, rest, hipMemcpyDeviceToDevice));
                }
                else
                {
                    stream.reserve(rest + 64);
                    SD_HIP(hipMemcpy(stream.p, base + consumed, rest, hipMemcpyDeviceToDevice));
                }
            }
            carry = rest;
            stream_base += (uint64_t)consumed;
            return written;
        }
        int64_t process(const int8_t *d_in, size_t n, unsigned char *d_out, size_t cap_frames)
        {
            SD_HIP(hipSetDevice(cfg.device));
            descs.clear();
            int64_t written = 0;
            size_t off = 0;
            do
            { // (the output does not depend on how the stream is cut: a long call is walked in pieces that bound the correlation table)
                const size_t m = std::min(n - off, (size_t)CT_READS * dec.g.F);
                written += piece(d_in + off, m, d_out + (size_t)written * frame_bytes, cap_frames - (size_t)written);
                off += m;
            } while (off < n);
            SD_HIP(hipDeviceSynchronize());
            return written;
        }
        size_t frames_bound(size_t n) const { return (carry + n) / dec.g.F + 1; } // frames a call of n bytes can write
    };

    inline void ct_check_unit(int rate, int base)
    {
        CtGeom g;
        if (rate < 0 || rate > 3)
            throw HipError("Invalid Turbo Rate!");
        if (!ct_geometry(rate, base, g))
            throw HipError("Turbo Base must be 223, 446, 892 or 1115!");
    }
} // namespace sdhip

extern "C"
{
    void sdhip_ccsds_turbo_cfg_default(sdhip_ccsds_turbo_cfg *c)
    {
        memset(c, 0, sizeof(*c));
        c->rate = SDHIP_CCSDS_TURBO_RATE_1_2;
        c->base = 223;
        c->iterations = 10;
        c->device = 0;
    }
    void *sdhip_ccsds_turbo_create(const sdhip_ccsds_turbo_cfg *c)
    {
        try
        {
            return new sdhip::CcsdsTurbo(*c);
        }
        catch (const std::exception &e)
        {
            sdhip::set_error(e.what());
            return nullptr;
        }
    }
    void sdhip_ccsds_turbo_destroy(void *h) { delete (sdhip::CcsdsTurbo *)h; }
    int sdhip_ccsds_turbo_frame_bytes(void *h) { return ((sdhip::CcsdsTurbo *)h)->frame_bytes; }
    int64_t sdhip_ccsds_turbo_process_dev(void *h, const int8_t *d_soft, size_t n, uint8_t *d_frames, size_t cap_frames)
    {
        try
        {
            return ((sdhip::CcsdsTurbo *)h)->process(d_soft, n, d_frames, cap_frames);
        }
        catch (const std::exception &e)
        {
            sdhip::set_error(e.what());
            return -1;
        }
    }
    int sdhip_ccsds_turbo_push(void *h, const int8_t *soft, size_t n)
    {
        try
        {
            sdhip::CcsdsTurbo *e = (sdhip::CcsdsTurbo *)h;
            SD_HIP(hipSetDevice(e->cfg.device));
            if (n == 0)
                return 0;
            sdhip::DevBuf<int8_t> din;
            sdhip::DevBuf<unsigned char> dout;
            const size_t cap = e->frames_bound(n);
            din.reserve(n);
            dout.reserve(cap * e->frame_bytes);
            SD_HIP(hipMemcpy(din.p, soft, n, hipMemcpyHostToDevice));
            const int64_t k = e->process(din.p, n, dout.p, cap);
            if (k > 0)
            {
                std::vector<unsigned char> v((size_t)k * e->frame_bytes);
                SD_HIP(hipMemcpy(v.data(), dout.p, v.size(), hipMemcpyDeviceToHost));
                e->outq.push_back(std::move(v));
            }
            return 0;
        }
        catch (const std::exception &e)
        {
            sdhip::set_error(e.what());
            return -1;
        }
    }
    int64_t sdhip_ccsds_turbo_pull(void *h, uint8_t *frames, size_t cap_frames)
    {
        sdhip::CcsdsTurbo *e = (sdhip::CcsdsTurbo *)h;
        const size_t fb = (size_t)e->frame_bytes;
        size_t got = 0;
        while (got < cap_frames && !e->outq.empty())
        {
            std::vector<unsigned char> &v = e->outq.front();
            const size_t have = v.size() / fb, take = std::min(have, cap_frames - got);
            memcpy(frames + got * fb, v.data(), take * fb);
            got += take;
            if (take == have)
                e->outq.pop_front();
            else
                v.erase(v.begin(), v.begin() + take * fb);
        }
        return (int64_t)got;
    }
    int sdhip_ccsds_turbo_get_stats(void *h, sdhip_ccsds_turbo_stats *st)
    {
        *st = ((sdhip::CcsdsTurbo *)h)->stats;
        return 0;
    }
    int64_t sdhip_ccsds_turbo_get_descs(void *h, sdhip_ccsds_turbo_desc *out, size_t cap)
    {
        const std::vector<sdhip_ccsds_turbo_desc> &d = ((sdhip::CcsdsTurbo *)h)->descs;
        const size_t k = std::min(cap, d.size());
        if (out && k)
            memcpy(out, d.data(), k * sizeof(sdhip_ccsds_turbo_desc));
        return (int64_t)d.size();
    }
    int sdhip_ccsds_turbo_interleaver(int base, int *out)
    {
        if (!(base == 223 || base == 446 || base == 892 || base == 1115))
        {
            sdhip::set_error("Turbo Base must be 223, 446, 892 or 1115!");
            return -1;
        }
        sdhip::ct_interleaver(base, out);
        return base * 8;
    }
    int sdhip_ccsds_turbo_asm(int rate, float *out192)
    {
        if (rate < 0 || rate > 3)
        {
            sdhip::set_error("Invalid Turbo Rate!");
            return -1;
        }
        const sdhip::CtAsm a = sdhip::ct_asm(rate);
        memcpy(out192, a.w, sizeof(a.w));
        sdhip::CtGeom g;
        sdhip::ct_geometry(rate, 223, g);
        return g.A;
    }
    int64_t sdhip_op_ccsds_turbo_correlate(int device, int rate, const int8_t *d_soft, size_t n, float *d_cor)
    {
        try
        {
            sdhip::ct_check_unit(rate, 223);
            sdhip::CtGeom g;
            sdhip::ct_geometry(rate, 223, g);
            if (n < (size_t)g.A)
                return 0;
            SD_HIP(hipSetDevice(device));
            const long long npos = (long long)n - g.A + 1;
            hipLaunchKernelGGL(sdhip::k_ct_correlate, dim3((unsigned)((npos + 255) / 256)), dim3(256), 0, nullptr, d_soft, (long long)n, sdhip::ct_asm(rate), g.A, d_cor);
            SD_HIP(hipDeviceSynchronize());
            return npos;
        }
        catch (const std::exception &e)
        {
            sdhip::set_error(e.what());
            return -1;
        }
    }
    int sdhip_op_ccsds_turbo_bcjr(int device, int rate, int base, int code, const double *d_stream, int nframes, double *d_msgs)
    {
        try
        {
            sdhip::ct_check_unit(rate, base);
            if ((code != 0 && code != 1) || nframes < 0)
                throw sdhip::HipError("ccsds_turbo: the constituent code is 0 (upper) or 1 (lower)");
            SD_HIP(hipSetDevice(device));
            sdhip::CtDecoder dec(rate, base);
            if (nframes > dec.piece)
                throw sdhip::HipError("ccsds_turbo: too many frames for one constituent pass");
            if (nframes == 0)
                return 0;
            sdhip::CtIn in{};
            in.mode = 2;
            in.cs = d_stream;
            in.stride = (code ? dec.g.nl : dec.g.nu) * dec.g.steps;
            dec.scratch(nframes);
            SD_HIP(hipMemcpy(dec.d_msgs.p, d_msgs, (size_t)nframes * 2 * dec.g.L * sizeof(double), hipMemcpyDeviceToDevice));
            dec.bcjr(in, code, 0, nframes, nullptr, 0, nullptr);
            SD_HIP(hipMemcpy(d_msgs, dec.d_msgs.p, (size_t)nframes * 2 * dec.g.L * sizeof(double), hipMemcpyDeviceToDevice));
            SD_HIP(hipDeviceSynchronize());
            return 0;
        }
        catch (const std::exception &e)
        {
            sdhip::set_error(e.what());
            return -1;
        }
    }
    int sdhip_op_ccsds_turbo_decode(int device, int rate, int base, int iterations, const float *d_codewords, int nframes, uint8_t *d_bits)
    {
        try
        {
            sdhip::ct_check_unit(rate, base);
            if (iterations < 1 || nframes < 0)
                throw sdhip::HipError("ccsds_turbo: turbo_iters must be at least 1");
            SD_HIP(hipSetDevice(device));
            sdhip::CtDecoder dec(rate, base);
            sdhip::CtIn in{};
            in.mode = 1;
            in.cw = d_codewords;
            in.stride = dec.g.wire * dec.g.steps;
            dec.decode(in, nframes, iterations, d_bits);
            SD_HIP(hipDeviceSynchronize());
            return 0;
        }
        catch (const std::exception &e)
        {
            sdhip::set_error(e.what());
            return -1;
        }
    }
}
