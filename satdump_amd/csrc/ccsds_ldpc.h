// ccsds_ldpc.h -- CCSDSLDPCDecoderModule::process() (src-core/pipeline/modules/ccsds/module_ccsds_ldpc_decoder.cpp:134-277) for "ldpc_rate": "7/8": a soft
// stream of 8192-byte frames (32-bit ASM + the (8176, 7154) code shortened to 8160 bits) -> CorrelatorGeneric -> rotate_soft / OQPSK Q shift ->
// derand_ccsds_soft -> CCSDSLDPC::decode over LDPCDecoderGeneric -> repacked frames behind the ASM, or ("internal_stream") the first 7136 bits of every
// codeword into the ASM deframer. Included from lrpt_decoder.hip, which owns the correlator-chain pattern this follows. gfx950, wave64.
//   k_cl_correlate  thread per stream position: CorrelatorGeneric::correlate's inner loop (generic_correlator.cpp:211-226) -- soft * (1 / 63) in float, the 32-term
//                   dot product with each syncword table summed left to right from 0 without FMA, the first syncword that is strictly greater. A position's
//                   answer does not depend on which read it falls in, so it is computed once per position: 256 positions + a 31-sample halo in LDS per block.
//   k_cl_spec       workgroup per grid frame behind an origin: the read's decision, a range arg-max over that table (first maximum, strict > from 0)
//   k_cl_walk       follows the answers while they say 0, takes the first slide as a new origin (k_lrpt_walk's bookkeeping)
//   k_cl_chain      the serial walk for a stream that keeps sliding
//   k_cl_decode     workgroup per codeword: frame preparation fused into the load (rotation.cpp:4-58, the module's Q shift :163-172, randomization.cpp:80-88,
//                   ccsds_ldpc.cpp:78-86), then LDPCDecoderGeneric::decode (ldpc_decoder_generic.cpp:69-194) with the 8176 int16 variable nodes and the
//                   check-to-variable messages in LDS. A new message is always +-min1 or +-min2, so a row's 32 messages are kept as min1, min2, 32 sign bits and
//                   32 is-min1 bits -- d_cn_to_vn_msgs exactly, in 12 bytes. Check nodes run in the reference's order wherever the order binds: rows that share no
//                   variable node commute, so the rows are cut into dependency levels (host, from the row list, at create time) with a barrier between levels; a
//                   row runs on 32 lanes, min1 / min2 by DPP + one cross-row exchange, parity and the bit masks by ballot. Neighbouring variable nodes share a dword:
//                   they are written with 16-bit LDS stores.
// The engine is generic over the row list (rows -> column indices, degree <= 32, sizes up to the (8176, 7154) code's); only the rate 7/8 list is built here.
// Kept quirks: the module writes (uint8_t *)&sync of a uint32_t -- 1D FC CF 1A on a little-endian host (:252-256); the derandomiser is ~x, not -x; variable
// nodes 0-17 enter as 0 and the last two wire bytes are dropped; bits 8158 / 8159 of a direct frame come from a buffer the module never writes there (0 here);
// after a slide the frame keeps the phase / swap of the first window, it is not correlated again. The SIMD decoders of the simd_extensions plugin batch 8 / 16
// frames and differ where parity ^ msg == 0 (they give 0, this code +min): not emulated, the parity target is LDPCDecoderGeneric.
// internal_stream: the decoded bits go through the FEC engine's own ASM deframer (a ccsds_simple_psk_decoder handle on +-1 soft bits, no derandomiser, no RS),
// created to work in blocks of one codeword's 7136 data bits -- what the module hands its deframer per call -- so no bit ever waits inside it: a CADU leaves
// with the call that decodes its last bit, as in the module.
#pragma once
#include "../../include/sdhip.h"
#include "common.h"

#include <algorithm>
#include <cstring>
#include <deque>
#include <vector>

namespace sdhip
{
    constexpr int CL_F = 8192;          // d_ldpc_frame_size: soft bytes per read
    constexpr int CL_ASM = 32;          // d_ldpc_asm_size
    constexpr int CL_CW = 8160;         // d_ldpc_codeword_size: CCSDSLDPC::frame_length()
    constexpr int CL_DATA = 7136;       // d_ldpc_data_size
    constexpr int CL_POS = CL_F - CL_ASM; // positions a read correlates: 0 .. length - syncword_length - 1
    constexpr int CL_MAX_VN = 8176, CL_MAX_CN = 1022, CL_MAX_DEG = 32;
    constexpr int CL_NT = 512;          // k_cl_decode: 16 rows at a time
    constexpr int CL_PIECE = 2048;      // frames per internal round of a call (bounds the correlation table)

    struct ClSync
    {
        float w[4][32];
        int n;
    };
    struct ClDesc
    {
        long long start; // first soft byte of the frame in the stream handed to the chain
        int sync;        // syncword index (phase / swap: cl_phase)
        float cor;
    };
    struct ClSpec
    {
        int pos, sync;
        float cor;
    };

    __global__ __launch_bounds__(256) void k_cl_correlate(const int8_t *__restrict__ soft, long long n, ClSync sw, float *__restrict__ cor, unsigned char *__restrict__ idx)
    {
        __shared__ float conv[256 + 32];
        const int tid = (int)threadIdx.x;
        const long long base = (long long)blockIdx.x * 256;
        for (int i = tid; i < 256 + 31; i += 256)
        {
            const long long j = base + i;
            conv[i] = j < n ? (float)soft[j] * (1.0f / 63.0f) : 0.0f; // volk_8i_s32f_convert_32f(.., 127 / 2, ..)
        }
        __syncthreads();
        const long long p = base + tid;
        if (p + 32 > n)
            return;
        float best = 0.0f;
        int bi = 0;
        for (int s = 0; s < sw.n; s++)
        {
            float acc = 0.0f;
#pragma unroll
            for (int x = 0; x < 32; x++)
                acc = acc + conv[tid + x] * sw.w[s][x]; // (the library is built with -ffp-contract=off: multiply, then add)
            if (acc > best)
            {
                best = acc;
                bi = s;
            }
        }
        cor[p] = best;
        idx[p] = (unsigned char)bi;
    }

    // the greatest correlation first, the lowest position among equals; 0 = nothing positive
    __device__ __forceinline__ unsigned long long cl_key(float c, int p) { return c > 0.0f ? ((unsigned long long)__float_as_uint(c) << 32) | (unsigned)(0x7FFFFFFF - p) : 0ull; }
    template <int NT>
    __device__ __forceinline__ unsigned long long cl_block_max(unsigned long long v, unsigned long long *red)
    {
        const int tid = (int)threadIdx.x;
        red[tid] = v;
        __syncthreads();
        for (int s = NT / 2; s > 0; s >>= 1)
        {
            if (tid < s)
            {
                const unsigned long long a = red[tid], b = red[tid + s];
                red[tid] = a > b ? a : b;
            }
            __syncthreads();
        }
        const unsigned long long r = red[0];
        __syncthreads();
        return r;
    }
    // one read at o: `cor = 0; for i: if (corr > cor) ...` over the per-position answers
    template <int NT>
    __device__ __forceinline__ ClSpec cl_read_decision(const float *__restrict__ cor, const unsigned char *__restrict__ idx, long long o, unsigned long long *red)
    {
        unsigned long long best = 0;
        for (int p = (int)threadIdx.x; p < CL_POS; p += NT)
        {
            const unsigned long long k = cl_key(cor[o + p], p);
            best = best > k ? best : k;
        }
        best = cl_block_max<NT>(best, red);
        if (best == 0)
            return ClSpec{0, 0, 0.0f};
        const int pos = 0x7FFFFFFF - (int)(unsigned)(best & 0xFFFFFFFFull);
        return ClSpec{pos, (int)idx[o + pos], __uint_as_float((unsigned)(best >> 32))};
    }

    __global__ __launch_bounds__(256) void k_cl_spec(const float *__restrict__ cor, const unsigned char *__restrict__ idx, long long origin, ClSpec *spec, int npos)
    {
        __shared__ unsigned long long red[256];
        const int k = (int)blockIdx.x;
        if (k >= npos)
            return;
        const ClSpec s = cl_read_decision<256>(cor, idx, origin + (long long)k * CL_F, red);
        if (threadIdx.x == 0)
            spec[k] = s;
    }
    // state[0] = frames so far, state[1] = 1 when the stream is used up (or the slid frame is not complete yet), consumed = where the chain stands
    __global__ __launch_bounds__(1024) void k_cl_walk(const ClSpec *__restrict__ spec, int npos, long long n, long long origin, ClDesc *descs, int max_frames, int *state,
                                                       long long *consumed, ClSpec *pend)
    {
        __shared__ int s_first;
        const int tid = (int)threadIdx.x;
        const int cnt0 = state[0];
        const long long fit = (n - origin) / CL_F;
        int limit = npos;
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
            descs[cnt0 + k] = ClDesc{origin + (long long)k * CL_F, spec[k].sync, spec[k].cor};
        if (tid == 0)
        {
            int cnt = cnt0 + first, done = 1;
            long long o = origin + (long long)first * CL_F;
            if (first < limit)
            { // the first slide: `pos` more bytes are read behind the window, the frame keeps the window's syncword; the next read starts behind it
                const ClSpec sp = spec[first];
                if (o + sp.pos + CL_F <= n)
                {
                    descs[cnt] = ClDesc{o + sp.pos, sp.sync, sp.cor};
                    cnt++;
                    o += sp.pos + CL_F;
                    done = (o + CL_F <= n && cnt < max_frames) ? 0 : 1;
                }
                else
                    *pend = sp; // the slid frame is not complete yet -- it stays for the next call; the module has its correlator's answer already
            }
            state[0] = cnt;
            state[1] = done;
            *consumed = o;
        }
    }
    __global__ __launch_bounds__(1024) void k_cl_chain(const float *__restrict__ cor, const unsigned char *__restrict__ idx, long long n, long long o0, ClDesc *descs, int max_frames,
                                                        int *count, long long *consumed, ClSpec *pend)
    {
        __shared__ unsigned long long red[1024];
        long long o = o0;
        int cnt = 0;
        while (o + CL_F <= n && cnt < max_frames)
        {
            const ClSpec s = cl_read_decision<1024>(cor, idx, o, red);
            if (s.pos != 0 && o + s.pos + CL_F > n)
            {
                if (threadIdx.x == 0)
                    *pend = s;
                break;
            }
            if (threadIdx.x == 0)
                descs[cnt] = ClDesc{o + s.pos, s.sync, s.cor};
            cnt++;
            o += s.pos + CL_F;
        }
        if (threadIdx.x == 0)
        {
            *count = cnt;
            *consumed = o;
        }
    }

    // ---- the decoder --------------------------------------------------------------------------------------------------------------------------------------
    struct ClCode
    {
        const unsigned short *cols; // [ncn][32] column indices of a row, 0xFFFF = no edge
        const unsigned short *order; // the rows, level after level (ascending inside a level)
        const int *lvl;              // [nlevels + 1] where each level starts in `order`
        int nlevels, ncn, nvn;
        int lead;                    // variable nodes in front of the wire bits that enter as 0 (18)
        int wire;                    // wire soft bytes placed behind them (8158)
    };
    struct ClPrep
    {
        int prepared;      // 1: `src` holds words of `stride` soft bytes as CCSDSLDPC::decode receives them (CL_CW); 0: the stream, frames named by descriptors
        int stride;        // prepared input and out_mode 0: bytes per word
        int constellation; // SDHIP_BPSK / QPSK / OQPSK
        int derand;
        unsigned pn[8];    // ccsds_soft_pn, bit i of the sequence = bit (i & 31) of word i >> 5
        int out_mode;      // 0: hard bits, a byte each, CL_CW per frame | 1: 1D FC CF 1A + 1020 packed bytes | 2: the first CL_DATA bits as +-1 soft bytes, frames butted
    };
    __device__ __forceinline__ void cl_phase(int constellation, int sync, int &phase, int &qshift)
    { // generic_correlator.cpp:233-261; the module hands `swap` to rotate_soft for BPSK / QPSK (always false there) and shifts Q itself for OQPSK
        qshift = 0;
        if (constellation == SDHIP_BPSK)
            phase = sync ? 2 : 0;
        else if (constellation == SDHIP_QPSK)
            phase = sync & 3;
        else
        {
            phase = sync == 0 ? 1 : (sync == 1 ? 3 : (sync == 2 ? 0 : 2));
            qshift = sync >> 1;
        }
    }
    // soft byte b of the frame at f after rotate_soft, the Q shift and the derandomiser
    __device__ __forceinline__ int cl_frame_byte(const int8_t *__restrict__ f, int b, int phase, int qshift, const ClPrep &pp)
    {
        int p = b >> 1;
        const int c = b & 1;
        int v = 0;
        if (qshift && c)
            p++; // Q of pair p is the turned Q of pair p + 1, a zero enters at the back
        if (p < CL_F / 2)
        {
            int a = f[2 * p], q = f[2 * p + 1];
            a = a == -128 ? -127 : a;
            q = q == -128 ? -127 : q;
            int ra = a, rq = q;
            if (phase == 1)
            {
                ra = q;
                rq = -a;
            }
            else if (phase == 2)
            {
                ra = -a;
                rq = -q;
            }
            else if (phase == 3)
            {
                ra = -q;
                rq = a;
            }
            v = c ? rq : ra;
        }
        if (pp.derand && b >= CL_ASM)
        {
            const int i = (b - CL_ASM) % 255;
            if ((pp.pn[i >> 5] >> (i & 31)) & 1u)
                v = (int)(signed char)~v; // ~x on an int8
        }
        return v;
    }
    // (min1, min2) of two disjoint sets, each packed min1 | min2 << 16
    __device__ __forceinline__ unsigned cl_min2(unsigned a, unsigned b)
    {
        const unsigned a1 = a & 0xFFFFu, a2 = a >> 16, b1 = b & 0xFFFFu, b2 = b >> 16;
        const unsigned lo = min(a1, b1), hi = max(a1, b1);
        return lo | (min(hi, min(a2, b2)) << 16);
    }

    __global__ __launch_bounds__(CL_NT) void k_cl_decode(const int8_t *__restrict__ src, const ClDesc *__restrict__ descs, int nframes, ClCode code, ClPrep pp, int iterations,
                                                          unsigned char *__restrict__ out, int *__restrict__ corrections)
    {
        __shared__ short s_vn[CL_MAX_VN];
        __shared__ unsigned s_mm[CL_MAX_CN], s_sg[CL_MAX_CN], s_im[CL_MAX_CN];
        __shared__ int s_corr;
        const int f = (int)blockIdx.x, tid = (int)threadIdx.x;
        if (f >= nframes)
            return;
        int phase = 0, qshift = 0;
        const int8_t *frame;
        if (pp.prepared)
            frame = src + (size_t)f * pp.stride;
        else
        {
            const ClDesc d = descs[f];
            frame = src + d.start;
            cl_phase(pp.constellation, d.sync, phase, qshift);
        }
        auto input = [&](int v) -> int { // depunc_buffer_in[v]
            if (v < code.lead || v >= code.lead + code.wire)
                return 0;
            const int i = v - code.lead;
            return pp.prepared ? (int)frame[i] : cl_frame_byte(frame, CL_ASM + i, phase, qshift, pp);
        };
        for (int v = tid; v < code.nvn; v += CL_NT)
            s_vn[v] = (short)input(v);
        for (int r = tid; r < code.ncn; r += CL_NT)
        {
            s_mm[r] = 0;
            s_sg[r] = 0;
            s_im[r] = 0;
        }
        if (tid == 0)
            s_corr = 0;
        __syncthreads();
        const int l32 = tid & 31, half = (tid >> 5) & 1, sub = tid >> 5;
        for (int it = 0; it < iterations; it++)
            for (int lv = 0; lv < code.nlevels; lv++)
            {
                const int lo = code.lvl[lv], hi = code.lvl[lv + 1];
                for (int base = lo; base < hi; base += CL_NT / 32)
                { // generic_cn_kernel of 16 rows that share no variable node, a row per half wave (the trip count is the workgroup's: the collectives below meet whole waves)
                    const int r = base + sub;
                    const bool active = r < hi;
                    const int row = active ? (int)code.order[r] : 0;
                    const unsigned col = active ? (unsigned)code.cols[row * CL_MAX_DEG + l32] : 0xFFFFu;
                    const bool edge = col != 0xFFFFu;
                    const unsigned mm = active ? s_mm[row] : 0u, sg = active ? s_sg[row] : 0u, im = active ? s_im[row] : 0u;
                    const int old_mag = (int)(((im >> l32) & 1u) ? (mm >> 16) : (mm & 0xFFFFu));
                    const int old = ((sg >> l32) & 1u) ? -old_mag : old_mag;
                    const int msg = edge ? (int)s_vn[edge ? col : 0] - old : 0; // d_vns_to_cn_msgs
                    const unsigned a = (unsigned)(msg < 0 ? -msg : msg);
                    unsigned m = (edge ? a : 0xFFFFu) | 0xFFFF0000u;
                    m = cl_min2(m, dpp_mov<0xB1>(m));
                    m = cl_min2(m, dpp_mov<0x4E>(m));
                    m = cl_min2(m, dpp_mov<0x141>(m));
                    m = cl_min2(m, dpp_mov<0x140>(m));
                    m = cl_min2(m, (unsigned)__shfl_xor((int)m, 16));
                    const unsigned min1 = min(m & 0xFFFFu, 255u), min2 = min(m >> 16, 255u); // both start at UINT8_MAX
                    const unsigned negs = (unsigned)(__ballot(edge && msg < 0) >> (32 * half));
                    const unsigned deg = (unsigned)__popc((unsigned)(__ballot(edge) >> (32 * half)));
                    const unsigned par = ((unsigned)__popc(negs) ^ deg) & 1u; // the sign bit of `parity` (complemented first for an odd degree)
                    const bool eq = edge && a == min1;
                    const int mag = (int)(eq ? min2 : min1);
                    const bool neg = ((par ^ (msg < 0 ? 1u : 0u)) & 1u) != 0; // sign = (parity ^ msg) >> 15
                    const int new_msg = neg ? -mag : mag;
                    if (edge)
                        s_vn[col] = (short)(new_msg + msg); // a 16-bit store: the neighbour in the dword belongs to another row
                    const unsigned nsg = (unsigned)(__ballot(edge && neg) >> (32 * half));
                    const unsigned nim = (unsigned)(__ballot(eq) >> (32 * half));
                    if (active && l32 == 0)
                    {
                        s_mm[row] = min1 | (min2 << 16);
                        s_sg[row] = nsg;
                        s_im[row] = nim;
                    }
                }
                __syncthreads();
            }
        // hard decision, corrections over the first nvn - ncn positions against in > 0
        int cnt = 0;
        for (int v = tid; v < code.nvn - code.ncn; v += CL_NT)
            cnt += ((s_vn[v] >= 0) != (input(v) > 0)) ? 1 : 0;
        if (cnt)
            atomicAdd(&s_corr, cnt);
        if (pp.out_mode == 0)
        {
            unsigned char *o = out + (size_t)f * pp.stride;
            for (int j = tid; j < pp.stride; j += CL_NT)
                o[j] = j < code.wire ? (unsigned char)(s_vn[code.lead + j] >= 0 ? 1 : 0) : (unsigned char)0;
        }
        else if (pp.out_mode == 1)
        {
            unsigned char *o = out + (size_t)f * (CL_CW / 8 + 4);
            for (int k = tid; k < CL_CW / 8 + 4; k += CL_NT)
            {
                unsigned b = 0;
                if (k < 4)
                    b = k == 0 ? 0x1Du : (k == 1 ? 0xFCu : (k == 2 ? 0xCFu : 0x1Au));
                else
                    for (int q = 0; q < 8; q++)
                    {
                        const int j = (k - 4) * 8 + q;
                        b = (b << 1) | ((j < code.wire && s_vn[code.lead + j] >= 0) ? 1u : 0u);
                    }
                o[k] = (unsigned char)b;
            }
        }
        else
        {
            signed char *o = reinterpret_cast<signed char *>(out) + (size_t)f * CL_DATA;
            for (int j = tid; j < CL_DATA; j += CL_NT)
                o[j] = (signed char)(s_vn[code.lead + j] >= 0 ? 1 : -1);
        }
        __syncthreads();
        if (tid == 0)
            corrections[f] = s_corr;
    }

    // ---- host ------------------------------------------------------------------------------------------------------------------------------------------------
    // the constructor's tables, generic_correlator.cpp:7-64. rotate_float_buf multiplies by complex_t(cosf(phase), sinf(phase)) with phase = deg * 0.01745329:
    // the six floats glibc returns there, as literals (tests/golden/ldpc holds the reference's tables)
    inline ClSync cl_syncwords(int constellation)
    {
        const unsigned asm32 = 0x1ACFFC1Du;
        unsigned char bits[32], delayed[32];
        for (int i = 0; i < 32; i++)
            delayed[i] = bits[i] = (unsigned char)((asm32 >> (31 - i)) & 1u);
        unsigned char last_q = 0; // "Syncword if we delayed the wrong phase"
        for (int i = 0; i < 16; i++)
        {
            const unsigned char back = delayed[i * 2 + 1];
            delayed[i * 2 + 1] = last_q;
            last_q = back;
        }
        const float C90 = 0x1.a22168p-23f, S90 = 1.0f, C180 = -1.0f, S180 = 0x1.a22168p-22f, C270 = -0x1.f3321ep-22f, S270 = -1.0f;
        ClSync s;
        memset(&s, 0, sizeof(s));
        auto modulate = [&](int k, const unsigned char *b) {
            for (int i = 0; i < 32; i++)
                s.w[k][i] = b[i] ? 1.0f : -1.0f;
        };
        auto rotate = [&](int k, float c, float sn) { // complex_t::operator*
            for (int i = 0; i < 16; i++)
            {
                const float re = s.w[k][2 * i], im = s.w[k][2 * i + 1];
                s.w[k][2 * i] = (re * c) - (im * sn);
                s.w[k][2 * i + 1] = (im * c) + (re * sn);
            }
        };
        if (constellation == SDHIP_BPSK)
        {
            s.n = 2;
            modulate(0, bits);
            modulate(1, bits);
            rotate(1, C180, S180);
        }
        else if (constellation == SDHIP_QPSK)
        {
            s.n = 4;
            for (int k = 0; k < 4; k++)
                modulate(k, bits);
            rotate(1, C90, S90);
            rotate(2, C180, S180);
            rotate(3, C270, S270);
        }
        else
        {
            s.n = 4;
            modulate(0, bits);
            modulate(1, bits);
            modulate(2, delayed);
            modulate(3, delayed);
            rotate(0, C90, S90);
            rotate(1, C270, S270);
            rotate(3, C180, S180);
        }
        return s;
    }

    // ccsds_78::make_r78_code (make_ccsds.cpp:394-433): two rows of sixteen 511 x 511 circulants of weight two; the first-row positions of CCSDS 131.1-O-2
    inline std::vector<std::vector<int>> cl_rows_r78()
    {
        static const unsigned short circ[2][16][2] = {
            {{0, 176}, {12, 239}, {0, 352}, {24, 431}, {0, 392}, {151, 409}, {0, 351}, {9, 359}, {0, 307}, {53, 329}, {0, 207}, {18, 281}, {0, 399}, {202, 457}, {0, 247}, {36, 261}},
            {{99, 471}, {130, 473}, {198, 435}, {260, 478}, {215, 420}, {282, 481}, {48, 396}, {193, 445}, {273, 430}, {302, 451}, {96, 379}, {191, 386}, {244, 467}, {364, 470}, {51, 382}, {192, 414}}};
        std::vector<std::vector<int>> rows(1022);
        for (int by = 0; by < 2; by++)
            for (int r = 0; r < 511; r++)
                for (int bx = 0; bx < 16; bx++)
                    for (int k = 0; k < 2; k++)
                        rows[by * 511 + r].push_back(511 * bx + (circ[by][bx][k] + r) % 511);
        return rows;
    }

    // The decoder for one row list: the rows in device memory and their level schedule. Row r must follow every earlier row it shares a variable node with and
    // nothing else: level(r) = 1 + the greatest level among those rows, rows of a level in ascending order.
    struct ClDecoder
    {
        DevBuf<unsigned short> d_cols, d_order;
        DevBuf<int> d_lvl;
        ClCode code{};
        std::vector<int> level_sizes;
        std::vector<unsigned short> schedule; // host copy of `order`

        ClDecoder(const std::vector<std::vector<int>> &rows, int nvn, int lead, int wire)
        {
            const int ncn = (int)rows.size();
            if (ncn > CL_MAX_CN || nvn > CL_MAX_VN || lead + wire > nvn)
                throw HipError("ccsds ldpc: the code does not fit the decoder kernel");
            std::vector<unsigned short> cols((size_t)ncn * CL_MAX_DEG, 0xFFFFu);
            std::vector<int> last(nvn, -1), level(ncn, 0);
            int nlevels = 0;
            for (int r = 0; r < ncn; r++)
            {
                if ((int)rows[r].size() > CL_MAX_DEG)
                    throw HipError("ccsds ldpc: a check node of more than 32 edges");
                int lv = 0;
                for (size_t k = 0; k < rows[r].size(); k++)
                {
                    const int c = rows[r][k];
                    if (c < 0 || c >= nvn)
                        throw HipError("ccsds ldpc: column index out of range");
                    for (size_t j = 0; j < k; j++)
                        if (rows[r][j] == c)
                            throw HipError("ccsds ldpc: a column twice in one row");
                    cols[(size_t)r * CL_MAX_DEG + k] = (unsigned short)c;
                    lv = std::max(lv, last[c] + 1);
                }
                for (int c : rows[r])
                    last[c] = lv;
                level[r] = lv;
                nlevels = std::max(nlevels, lv + 1);
            }
            std::vector<int> lvl(nlevels + 1, 0);
            for (int r = 0; r < ncn; r++)
                lvl[level[r] + 1]++;
            for (int l = 0; l < nlevels; l++)
            {
                level_sizes.push_back(lvl[l + 1]);
                lvl[l + 1] += lvl[l];
            }
            std::vector<unsigned short> order(ncn);
            std::vector<int> fill(lvl.begin(), lvl.end() - 1);
            for (int r = 0; r < ncn; r++)
                order[fill[level[r]]++] = (unsigned short)r;
            schedule = order;
            d_cols.reserve(cols.size());
            d_order.reserve(order.size());
            d_lvl.reserve(lvl.size());
            SD_HIP(hipMemcpy(d_cols.p, cols.data(), cols.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
            SD_HIP(hipMemcpy(d_order.p, order.data(), order.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
            SD_HIP(hipMemcpy(d_lvl.p, lvl.data(), lvl.size() * sizeof(int), hipMemcpyHostToDevice));
            code = ClCode{d_cols.p, d_order.p, d_lvl.p, nlevels, ncn, nvn, lead, wire};
        }
        void launch(const int8_t *src, const ClDesc *descs, int nframes, const ClPrep &pp, int iterations, unsigned char *out, int *corrections)
        {
            if (nframes <= 0)
                return;
            ProfScope _ps("k_cl_decode", nullptr);
            hipLaunchKernelGGL(k_cl_decode, dim3((unsigned)nframes), dim3(CL_NT), 0, nullptr, src, descs, nframes, code, pp, iterations, out, corrections);
        }
    };
    inline void cl_soft_pn(unsigned pn[8])
    { // ccsds_soft_pn (randomization.cpp:39): h(x) = x^8 + x^7 + x^5 + x^3 + 1 from all ones, a bit per entry
        memset(pn, 0, 8 * sizeof(unsigned));
        unsigned reg = 0xFF;
        for (int i = 0; i < 255; i++)
        {
            if (reg & 1u)
                pn[i >> 5] |= 1u << (i & 31);
            const unsigned fb = ((reg >> 0) ^ (reg >> 3) ^ (reg >> 5) ^ (reg >> 7)) & 1u;
            reg = (reg >> 1) | (fb << 7);
        }
    }
    inline void cl_launch_correlate(const int8_t *d_soft, long long n, const ClSync &sw, float *d_cor, unsigned char *d_idx)
    {
        if (n < 32)
            return;
        ProfScope _ps("k_cl_correlate", nullptr);
        const long long npos = n - 31;
        hipLaunchKernelGGL(k_cl_correlate, dim3((unsigned)((npos + 255) / 256)), dim3(256), 0, nullptr, d_soft, n, sw, d_cor, d_idx);
    }

    struct CcsdsLdpc
    {
        sdhip_ccsds_ldpc_cfg cfg;
        sdhip_ccsds_ldpc_stats stats{};
        ClSync sync;
        ClPrep prep{};
        ClDecoder dec;
        void *fec = nullptr; // internal_stream: the ASM deframer (a ccsds_simple_psk_decoder handle)
        int frame_bytes;
        DevBuf<int8_t> stream;
        size_t carry = 0;
        uint64_t stream_base = 0; // stream position of stream[0]
        DevBuf<float> d_cor;
        DevBuf<unsigned char> d_idx, d_bits;
        DevBuf<ClDesc> d_desc;
        DevBuf<ClSpec> d_spec, d_pend;
        DevBuf<int> d_state, d_cnt, d_corr;
        DevBuf<long long> d_consumed;
        std::vector<sdhip_ccsds_ldpc_desc> descs; // of the last call
        std::deque<std::vector<unsigned char>> outq;

        static const sdhip_ccsds_ldpc_cfg &checked(const sdhip_ccsds_ldpc_cfg &c)
        {
            if (c.constellation != SDHIP_BPSK && c.constellation != SDHIP_QPSK && c.constellation != SDHIP_OQPSK)
                throw HipError("CCSDS LDPC Decoder : invalid constellation type!");
            if (c.rate != SDHIP_CCSDS_LDPC_RATE_7_8)
                throw HipError("ccsds_ldpc: only ldpc_rate 7/8 runs on the device (the AR4JA rates 1/2, 2/3, 4/5 stay on the CPU module)");
            if (c.iterations < 0)
                throw HipError("ccsds_ldpc: ldpc_iterations must not be negative");
            if (c.internal_stream && (c.internal_cadu_size <= 32 || c.internal_cadu_size % 8 != 0))
                throw HipError("ccsds_ldpc: internal_cadu_size must be a multiple of 8 (padded CADUs stay on the CPU module)");
            return c;
        }
        explicit CcsdsLdpc(const sdhip_ccsds_ldpc_cfg &c) : cfg(checked(c)), dec(((void)hipSetDevice(c.device), cl_rows_r78()), 8176, 18, 8158)
        {
            sync = cl_syncwords(cfg.constellation);
            prep.prepared = 0;
            prep.constellation = cfg.constellation;
            prep.derand = cfg.derandomize ? 1 : 0;
            cl_soft_pn(prep.pn);
            prep.out_mode = cfg.internal_stream ? 2 : 1;
            frame_bytes = cfg.internal_stream ? cfg.internal_cadu_size / 8 : CL_CW / 8 + 4;
            if (cfg.internal_stream)
            {
                sdhip_fec_cfg fc;
                sdhip_fec_cfg_default(&fc);
                fc.decoder = SDHIP_DEC_SIMPLE_PSK;
                fc.constellation = SDHIP_BPSK;
                fc.cadu_size = cfg.internal_cadu_size;
                fc.nrzm = 0;
                fc.derandomize = 0;
                fc.rs_i = 0;
                fc.rs_usecheck = 0;
                fc.asm_sync = cfg.internal_asm;
                fc.device = cfg.device;
                fec = sdhip_fec_create_bit_deframer(&fc, CL_DATA);
                if (!fec)
                    throw HipError(std::string("ccsds_ldpc: the deframer: ") + sdhip_last_error());
            }
            d_state.reserve(2);
            d_cnt.reserve(1);
            d_consumed.reserve(1);
            stats.deframer_state = 2;
        }
        ~CcsdsLdpc()
        {
            if (fec)
                sdhip_fec_destroy(fec);
        }

        // the module's loop over the bytes at hand: descriptors for every complete frame, *consumed = where the next read starts
        int chain(const int8_t *base, long long total, long long *consumed_out, ClSpec *pending_read)
        {
            d_pend.reserve(1);
            SD_HIP(hipMemsetAsync(d_pend.p, 0, sizeof(ClSpec), nullptr)); // pos 0: no read waits for its slide
            d_cor.reserve((size_t)total);
            d_idx.reserve((size_t)total);
            cl_launch_correlate(base, total, sync, d_cor.p, d_idx.p);
            const int max_frames = (int)(total / CL_F) + 1;
            d_desc.reserve(max_frames);
            d_spec.reserve(max_frames);
            int nf = 0;
            long long consumed = 0;
            bool chained = false;
            {
                ProfScope _ps("k_cl_spec + k_cl_walk", nullptr);
                SD_HIP(hipMemsetAsync(d_state.p, 0, 2 * sizeof(int), nullptr));
                long long origin = 0;
                int st[2] = {0, 0};
                for (int round = 0; round < 6; round++)
                {
                    const int npos = (int)((total - origin) / CL_F);
                    if (npos <= 0)
                    {
                        st[1] = 1;
                        consumed = origin;
                        break;
                    }
                    hipLaunchKernelGGL(k_cl_spec, dim3((unsigned)npos), dim3(256), 0, nullptr, d_cor.p, d_idx.p, origin, d_spec.p, npos);
                    hipLaunchKernelGGL(k_cl_walk, dim3(1), dim3(1024), 0, nullptr, d_spec.p, npos, total, origin, d_desc.p, max_frames, d_state.p, d_consumed.p, d_pend.p);
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
            { // a stream that keeps sliding: the serial walk over what is left, behind the frames found so far
                ProfScope _ps("k_cl_chain", nullptr);
                int rest = 0;
                hipLaunchKernelGGL(k_cl_chain, dim3(1), dim3(1024), 0, nullptr, d_cor.p, d_idx.p, total, consumed, d_desc.p + nf, max_frames - nf, d_cnt.p, d_consumed.p, d_pend.p);
                SD_HIP(hipMemcpy(&rest, d_cnt.p, sizeof(int), hipMemcpyDeviceToHost));
                SD_HIP(hipMemcpy(&consumed, d_consumed.p, sizeof(long long), hipMemcpyDeviceToHost));
                nf += rest;
                stats.chain_serial++;
            }
            SD_HIP(hipMemcpy(pending_read, d_pend.p, sizeof(ClSpec), hipMemcpyDeviceToHost));
            *consumed_out = consumed;
            return nf;
        }

        // n more soft bytes (device, n <= CL_PIECE frames' worth); frames to d_out (room for cap_frames). Returns the frames written.
        int64_t piece(const int8_t *d_in, size_t n, unsigned char *d_out, size_t cap_frames)
        {
            stats.soft_in += n;
            const size_t total = carry + n;
            const int8_t *base = d_in;
            if (carry || total < (size_t)CL_F)
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
            if (total < (size_t)CL_F)
            {
                carry = total;
                return 0;
            }
            long long consumed = 0;
            ClSpec pending_read{0, 0, 0.0f};
            const int nf = chain(base, (long long)total, &consumed, &pending_read);
            int64_t written = 0;
            if (nf > 0)
            {
                d_corr.reserve(nf);
                std::vector<ClDesc> hd(nf);
                std::vector<int> hc(nf);
                if (cfg.internal_stream)
                {
                    d_bits.reserve((size_t)nf * CL_DATA);
                    dec.launch(base, d_desc.p, nf, prep, cfg.iterations, d_bits.p, d_corr.p);
                    written = sdhip_fec_process_dev(fec, reinterpret_cast<const int8_t *>(d_bits.p), (size_t)nf * CL_DATA, d_out, cap_frames);
                    if (written < 0)
                        throw HipError(std::string("ccsds_ldpc: the deframer: ") + sdhip_last_error());
                    sdhip_fec_stats fs;
                    sdhip_fec_get_stats(fec, &fs);
                    stats.deframer_state = fs.deframer_state;
                    SD_HIP(hipSetDevice(cfg.device));
                }
                else
                {
                    if ((size_t)nf > cap_frames)
                        throw HipError("ccsds_ldpc: frame output buffer too small");
                    dec.launch(base, d_desc.p, nf, prep, cfg.iterations, d_out, d_corr.p);
                    written = nf;
                }
                SD_HIP(hipMemcpy(hd.data(), d_desc.p, (size_t)nf * sizeof(ClDesc), hipMemcpyDeviceToHost));
                SD_HIP(hipMemcpy(hc.data(), d_corr.p, (size_t)nf * sizeof(int), hipMemcpyDeviceToHost));
                long long read_at = 0; // where the read that produced the frame started: the previous frame's end
                for (int f = 0; f < nf; f++)
                {
                    descs.push_back(sdhip_ccsds_ldpc_desc{stream_base + (uint64_t)hd[f].start, hd[f].sync, hd[f].cor, hc[f], hd[f].start == read_at ? 1 : 0});
                    read_at = hd[f].start + CL_F;
                }
                stats.frames_seen += nf;
                stats.frames_out += written;
                stats.correlator_lock = descs.back().locked;
                stats.correlator_corr = hd[nf - 1].cor;
                stats.ldpc_corr = hc[nf - 1];
            }
            if (pending_read.pos != 0)
            { // a read whose slide is not complete: the module has set these at correlate() already (module_ccsds_ldpc_decoder.cpp:147-149)
                stats.correlator_lock = 0;
                stats.correlator_corr = pending_read.cor;
            }
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
                const size_t m = std::min(n - off, (size_t)CL_PIECE * CL_F);
                written += piece(d_in + off, m, d_out + (size_t)written * frame_bytes, cap_frames - (size_t)written);
                off += m;
            } while (off < n);
            SD_HIP(hipDeviceSynchronize());
            return written;
        }
        size_t frames_bound(size_t n) const
        { // frames a call of n bytes can write
            const size_t cw = (carry + n) / CL_F + 1;
            return cfg.internal_stream ? (cw * CL_DATA) / (size_t)cfg.internal_cadu_size + 2 : cw;
        }
    };
} // namespace sdhip

extern "C"
{
    void sdhip_ccsds_ldpc_cfg_default(sdhip_ccsds_ldpc_cfg *c)
    {
        memset(c, 0, sizeof(*c));
        c->constellation = SDHIP_QPSK;
        c->rate = SDHIP_CCSDS_LDPC_RATE_7_8;
        c->block_size = 0;
        c->iterations = 10;
        c->derandomize = 1;
        c->internal_stream = 0;
        c->internal_cadu_size = 0;
        c->internal_asm = 0x1ACFFC1Du;
        c->device = 0;
    }
    void *sdhip_ccsds_ldpc_create(const sdhip_ccsds_ldpc_cfg *c)
    {
        try
        {
            return new sdhip::CcsdsLdpc(*c);
        }
        catch (const std::exception &e)
        {
            sdhip::set_error(e.what());
            return nullptr;
        }
    }
    void sdhip_ccsds_ldpc_destroy(void *h) { delete (sdhip::CcsdsLdpc *)h; }
    int sdhip_ccsds_ldpc_frame_bytes(void *h) { return ((sdhip::CcsdsLdpc *)h)->frame_bytes; }
    int64_t sdhip_ccsds_ldpc_process_dev(void *h, const int8_t *d_soft, size_t n, uint8_t *d_frames, size_t cap_frames)
    {
        try
        {
            return ((sdhip::CcsdsLdpc *)h)->process(d_soft, n, d_frames, cap_frames);
        }
        catch (const std::exception &e)
        {
            sdhip::set_error(e.what());
            return -1;
        }
    }
    int sdhip_ccsds_ldpc_push(void *h, const int8_t *soft, size_t n)
    {
        try
        {
            sdhip::CcsdsLdpc *e = (sdhip::CcsdsLdpc *)h;
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
    int64_t sdhip_ccsds_ldpc_pull(void *h, uint8_t *frames, size_t cap_frames)
    {
        sdhip::CcsdsLdpc *e = (sdhip::CcsdsLdpc *)h;
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
    int sdhip_ccsds_ldpc_get_stats(void *h, sdhip_ccsds_ldpc_stats *st)
    {
        *st = ((sdhip::CcsdsLdpc *)h)->stats;
        return 0;
    }
    int64_t sdhip_ccsds_ldpc_get_descs(void *h, sdhip_ccsds_ldpc_desc *out, size_t cap)
    {
        const std::vector<sdhip_ccsds_ldpc_desc> &d = ((sdhip::CcsdsLdpc *)h)->descs;
        const size_t k = std::min(cap, d.size());
        if (out && k)
            memcpy(out, d.data(), k * sizeof(sdhip_ccsds_ldpc_desc));
        return (int64_t)d.size();
    }
    int sdhip_ccsds_ldpc_syncwords(int constellation, float *out128)
    {
        if (constellation != SDHIP_BPSK && constellation != SDHIP_QPSK && constellation != SDHIP_OQPSK)
            return -1;
        const sdhip::ClSync s = sdhip::cl_syncwords(constellation);
        memcpy(out128, s.w, sizeof(s.w));
        return s.n;
    }
    int sdhip_ccsds_ldpc_levels(void *h, int *sizes, int cap)
    {
        const std::vector<int> &l = ((sdhip::CcsdsLdpc *)h)->dec.level_sizes;
        for (int i = 0; i < (int)l.size() && i < cap; i++)
            sizes[i] = l[i];
        return (int)l.size();
    }
    int sdhip_ccsds_ldpc_schedule(void *h, uint16_t *rows, int cap)
    {
        const std::vector<unsigned short> &o = ((sdhip::CcsdsLdpc *)h)->dec.schedule;
        for (int i = 0; i < (int)o.size() && i < cap; i++)
            rows[i] = o[i];
        return (int)o.size();
    }
    int sdhip_op_ccsds_ldpc_decode(int device, int rate, int iterations, const int8_t *d_codewords, int nframes, uint8_t *d_bits, int *d_corrections)
    {
        try
        {
            if (rate != SDHIP_CCSDS_LDPC_RATE_7_8)
                throw sdhip::HipError("ccsds_ldpc: only ldpc_rate 7/8 runs on the device (the AR4JA rates 1/2, 2/3, 4/5 stay on the CPU module)");
            if (iterations < 0 || nframes < 0)
                throw sdhip::HipError("ccsds_ldpc: ldpc_iterations must not be negative");
            SD_HIP(hipSetDevice(device));
            sdhip::ClDecoder dec(sdhip::cl_rows_r78(), 8176, 18, 8158);
            sdhip::ClPrep pp{};
            pp.prepared = 1;
            pp.stride = sdhip::CL_CW;
            pp.out_mode = 0;
            dec.launch(d_codewords, nullptr, nframes, pp, iterations, d_bits, d_corrections);
            SD_HIP(hipDeviceSynchronize());
            return 0;
        }
        catch (const std::exception &e)
        {
            sdhip::set_error(e.what());
            return -1;
        }
    }
    int sdhip_op_ldpc_generic_decode(int device, const uint16_t *rows, int ncn, int nvn, int iterations, const int8_t *d_words, int nwords, uint8_t *d_bits, int *d_corrections)
    {
        try
        {
            if (iterations < 0 || nwords < 0 || ncn <= 0 || nvn <= 0)
                throw sdhip::HipError("ccsds_ldpc: ldpc_iterations must not be negative");
            SD_HIP(hipSetDevice(device));
            std::vector<std::vector<int>> rl(ncn);
            for (int r = 0; r < ncn; r++)
                for (int k = 0; k < sdhip::CL_MAX_DEG; k++)
                    if (rows[r * sdhip::CL_MAX_DEG + k] != 0xFFFFu)
                        rl[r].push_back(rows[r * sdhip::CL_MAX_DEG + k]);
            sdhip::ClDecoder dec(rl, nvn, 0, nvn);
            sdhip::ClPrep pp{};
            pp.prepared = 1;
            pp.stride = nvn;
            pp.out_mode = 0;
            dec.launch(d_words, nullptr, nwords, pp, iterations, d_bits, d_corrections);
            SD_HIP(hipDeviceSynchronize());
            return 0;
        }
        catch (const std::exception &e)
        {
            sdhip::set_error(e.what());
            return -1;
        }
    }
    int64_t sdhip_op_generic_correlate(int device, int constellation, const int8_t *d_soft, size_t n, float *d_cor, uint8_t *d_sync)
    {
        try
        {
            if (constellation != SDHIP_BPSK && constellation != SDHIP_QPSK && constellation != SDHIP_OQPSK)
                throw sdhip::HipError("CCSDS LDPC Decoder : invalid constellation type!");
            if (n < 32)
                return 0;
            SD_HIP(hipSetDevice(device));
            sdhip::cl_launch_correlate(d_soft, (long long)n, sdhip::cl_syncwords(constellation), d_cor, d_sync);
            SD_HIP(hipDeviceSynchronize());
            return (int64_t)(n - 31);
        }
        catch (const std::exception &e)
        {
            sdhip::set_error(e.what());
            return -1;
        }
    }
}
