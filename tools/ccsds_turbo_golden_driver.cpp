// tools/ccsds_turbo_golden_driver.cpp -- TEST INFRASTRUCTURE ONLY: the driver tools/gen_ccsds_turbo_golden.py compiles (into a temporary directory, with the oracle's
// recorded flags -O2 -ffp-contract=off and ref_shim/) next to the reference's own sources, to record what ccsds_turbo_decoder computes as fixtures under
// tests/golden/turbo/. Nothing here is product code and nothing of it is committed in compiled form.
//
// It restates CCSDSTurboDecoderModule::process() (module_ccsds_turbo_decoder.cpp:139-257) over an in-memory stream, on the reference's own CCSDSTurbo (over
// libturbocodes.c / libconvcodes.c), derand_ccsds_soft and GenericCRC. The reads become a FIFO that the caller fills in pieces: a read that the FIFO cannot serve --
// the main read of a buffer, or the `pos` bytes behind a slide -- waits for the next piece, and the stream ends at the first incomplete read. The module's
// memmove(buf, buf + pos, pos) reads past its buffer when pos > F / 2; the bytes it fetches there are overwritten by the second read, so the restatement moves
// min(pos, F - pos) bytes and arrives at the same buffer. The module's last iteration at the end of a file (the previous buffer decoded again after a second
// derandomisation) is not restated.
// turboref_iterate restates turbo_decode's loop (libturbocodes.c:160-186) over convcode_extrinsic, so that the bits after every iteration and the a-priori arrays
// around each pass can be recorded, and so that the messages can be perturbed between the passes (which tells the decisions that hang on the last bits of exp / log).
// Built with -fno-access-control (d_pi, d_turbo and puncturing() are private) and -Dvolk_8i_s32f_convert_32f=volk_8i_s32f_convert_32f_u (the shim's name for
// VOLK's generic kernel).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include <volk/volk.h>

#include "common/codings/crc/crc_generic.h"
#include "common/codings/randomization.h"
#include "common/codings/turbo/ccsds_turbo.h"

namespace
{
    using codings::turbo::CCSDSTurbo;
    const char *const ASM_HEX[4] = {"034776C7272895B0", "25D5C0CE8990F6C9461BF79C", "034776C7272895B0FCB88938D8D76A4F", "25D5C0CE8990F6C9461BF79CDA2A3F31766F0936B9E40863"};
    int hexval(char c) { return c <= '9' ? c - '0' : c - 'A' + 10; }

    struct Desc
    {
        int64_t offset;
        int pos, swapped;
        float cor;
        int crc_ok;
    };
    struct Run
    {
        int d_turbo_base, d_turbo_iters;
        int d_asm_size, d_codeword_size, d_frame_size;
        float asm_softs[192];
        std::vector<int8_t> buffer_soft;
        std::vector<float> buffer_floats;
        CCSDSTurbo turbo_dec;
        codings::crc::GenericCRC crc_check;
        // the stream
        std::vector<int8_t> fifo;
        size_t rd = 0;
        int64_t stream_pos = 0;
        // a read in progress behind a slide
        bool sliding = false;
        int best_pos = 0;
        bool best_swapped = false;
        int64_t read_start = 0;
        // results
        bool locked = false, crc_lock = false;
        float cor = 0;
        std::vector<Desc> descs;
        std::vector<uint8_t> out;

        Run(int rate, int base, int iters)
            : d_turbo_base(base), d_turbo_iters(iters), turbo_dec((codings::turbo::turbo_base_t)base, (codings::turbo::turbo_rate_t)rate), crc_check(16, 0x1021, 0xFFFF, 0x0, false, false)
        {
            d_asm_size = (int)strlen(ASM_HEX[rate]) * 4;
            for (int i = 0; i < d_asm_size; i++)
                asm_softs[i] = ((hexval(ASM_HEX[rate][i / 4]) >> (3 - i % 4)) & 1) ? 1.0f : -1.0f;
            d_codeword_size = turbo_dec.codeword_length();
            d_frame_size = d_codeword_size + d_asm_size;
            buffer_soft.resize(d_frame_size);
            buffer_floats.resize(d_frame_size);
        }
        bool read_data(int8_t *dst, int n)
        {
            if (fifo.size() - rd < (size_t)n)
                return false;
            memcpy(dst, fifo.data() + rd, n);
            rd += n;
            stream_pos += n;
            return true;
        }
        void feed(const int8_t *soft, int64_t n)
        {
            fifo.erase(fifo.begin(), fifo.begin() + rd);
            rd = 0;
            fifo.insert(fifo.end(), soft, soft + n);
            for (;;)
            {
                if (!sliding)
                {
                    read_start = stream_pos;
                    if (!read_data(buffer_soft.data(), d_frame_size))
                        return;
                    volk_8i_s32f_convert_32f(buffer_floats.data(), buffer_soft.data(), 127, d_frame_size);
                    best_pos = 0;
                    float best_cor = 0;
                    best_swapped = false;
                    float corr_value = 0;
                    for (int pos = 0; pos < d_frame_size - d_asm_size; pos++)
                    {
                        volk_32f_x2_dot_prod_32f(&corr_value, &buffer_floats[pos], asm_softs, d_asm_size);
                        if (corr_value > best_cor)
                        {
                            best_cor = corr_value;
                            best_pos = pos;
                            best_swapped = false;
                        }
                        if (-corr_value > best_cor)
                        {
                            best_cor = -corr_value;
                            best_pos = pos;
                            best_swapped = true;
                        }
                    }
                    locked = best_pos == 0;
                    cor = best_cor;
                    if (best_pos != 0 && best_pos < d_frame_size)
                    {
                        std::memmove(buffer_soft.data(), &buffer_soft[best_pos], std::min(best_pos, d_frame_size - best_pos));
                        sliding = true;
                    }
                }
                if (sliding)
                {
                    if (!read_data(&buffer_soft[d_frame_size - best_pos], best_pos))
                        return;
                    sliding = false;
                }
                derand_ccsds_soft(&buffer_soft[d_asm_size], d_codeword_size);
                volk_8i_s32f_convert_32f(buffer_floats.data(), buffer_soft.data(), 127.0, d_frame_size);
                if (best_swapped)
                    for (int i = 0; i < d_frame_size; i++)
                        buffer_floats[i] = -buffer_floats[i];
                uint8_t output_frame_buffer[1115 + 4];
                turbo_dec.decode(&buffer_floats[d_asm_size], &output_frame_buffer[4], d_turbo_iters);
                output_frame_buffer[0] = 0x1a;
                output_frame_buffer[1] = 0xcf;
                output_frame_buffer[2] = 0xfc;
                output_frame_buffer[3] = 0x1d;
                uint16_t compu_crc = crc_check.compute(&output_frame_buffer[4], d_turbo_base - 2);
                uint16_t local_crc = output_frame_buffer[(d_turbo_base + 4) - 2] << 8 | output_frame_buffer[(d_turbo_base + 4) - 1];
                crc_lock = compu_crc == local_crc;
                if (crc_lock)
                    out.insert(out.end(), output_frame_buffer, output_frame_buffer + d_turbo_base + 4);
                descs.push_back(Desc{read_start, best_pos, best_swapped ? 1 : 0, cor, crc_lock ? 1 : 0});
            }
        }
    };

    // CCSDSTurbo::decode's depuncturing and turbo_decode's serial-to-parallel split, as they stand in ccsds_turbo.cpp:160-183 and libturbocodes.c:140-158
    void split(CCSDSTurbo &t, const float *codeword, std::vector<double> streams[2])
    {
        t.d_turbo.interleaver = t.d_pi;
        const int n = t.d_turbo.encoded_length;
        std::vector<double> dep(n);
        if (t.d_code_type == codings::turbo::RATE_1_2)
        {
            int j = 0;
            for (int i = 0; i < n; i++)
                dep[i] = t.puncturing(i) ? (double)codeword[j++] : 0.0;
        }
        else
            for (int i = 0; i < n; i++)
                dep[i] = codeword[i];
        t_convcode codes[2] = {t.d_turbo.upper_code, t.d_turbo.lower_code};
        for (int i = 0; i < 2; i++)
            streams[i].assign((size_t)codes[i].components * (t.d_turbo.packet_length + codes[i].memory), 0.0);
        int k = 0, c = 0, cw = 0;
        while (k < n)
        {
            for (int i = 0; i < codes[c].components; i++)
                streams[c][cw * codes[c].components + i] = dep[k++];
            c = (c + 1) % 2;
            cw = !c ? cw + 1 : cw;
        }
    }
}

extern "C"
{
    void *turboref_create(int rate, int base, int iters) { return new Run(rate, base, iters); }
    void turboref_destroy(void *h) { delete (Run *)h; }
    void turboref_feed(void *h, const int8_t *soft, int64_t n) { ((Run *)h)->feed(soft, n); }
    int64_t turboref_ndesc(void *h) { return (int64_t)((Run *)h)->descs.size(); }
    int64_t turboref_nout(void *h) { return (int64_t)((Run *)h)->out.size(); }
    int turboref_frame_size(void *h) { return ((Run *)h)->d_frame_size; }
    // offset[n], pos[n], swapped[n], cor[n], crc_ok[n]; out bytes; stats3 = {locked, crc_lock, a read waits for its slide}, cor1 = cor
    void turboref_results(void *h, int64_t *offset, int *pos, int *swapped, float *cor, int *crc_ok, uint8_t *out, int *stats3, float *cor1)
    {
        Run *r = (Run *)h;
        for (size_t i = 0; i < r->descs.size(); i++)
        {
            offset[i] = r->descs[i].offset;
            pos[i] = r->descs[i].pos;
            swapped[i] = r->descs[i].swapped;
            cor[i] = r->descs[i].cor;
            crc_ok[i] = r->descs[i].crc_ok;
        }
        memcpy(out, r->out.data(), r->out.size());
        stats3[0] = r->locked ? 1 : 0;
        stats3[1] = r->crc_lock ? 1 : 0;
        stats3[2] = r->sliding ? 1 : 0;
        *cor1 = r->cor;
    }
    // the module's correlation at every position p <= n - A, window by window
    void turboref_positions(void *h, const int8_t *soft, int64_t n, float *cor)
    {
        Run *r = (Run *)h;
        std::vector<float> f(n);
        volk_8i_s32f_convert_32f(f.data(), soft, 127, (unsigned)n);
        for (int64_t p = 0; p + r->d_asm_size <= n; p++)
            volk_32f_x2_dot_prod_32f(&cor[p], &f[p], r->asm_softs, r->d_asm_size);
    }
    void turboref_asm(void *h, float *out) { memcpy(out, ((Run *)h)->asm_softs, ((Run *)h)->d_asm_size * sizeof(float)); }
    void turboref_pi(int base, int *out)
    {
        CCSDSTurbo t((codings::turbo::turbo_base_t)base, codings::turbo::RATE_1_3);
        memcpy(out, t.d_pi, (size_t)base * 8 * sizeof(int));
    }
    int turboref_codeword_length(int rate, int base)
    {
        CCSDSTurbo t((codings::turbo::turbo_base_t)base, (codings::turbo::turbo_rate_t)rate);
        return t.codeword_length();
    }
    // CCSDSTurbo::encode: frame (base bytes) -> code bits, one per byte. encode() packs with `byte << 1 | bit`, so a last byte of fewer than 8 bits holds them in its low end.
    void turboref_encode(int rate, int base, const uint8_t *frame, uint8_t *bits)
    {
        CCSDSTurbo t((codings::turbo::turbo_base_t)base, (codings::turbo::turbo_rate_t)rate);
        const int n = t.codeword_length();
        std::vector<uint8_t> fr(frame, frame + base), cw(n / 8 + 2, 0);
        t.encode(fr.data(), cw.data());
        for (int i = 0; i < n; i++)
        {
            const int in_byte = (i / 8 == n / 8) ? n % 8 : 8;
            bits[i] = (cw[i / 8] >> (in_byte - 1 - i % 8)) & 1;
        }
    }
    // CCSDSTurbo::decode on n prepared float codewords -> information bits, one per byte
    void turboref_decode(int rate, int base, int iters, const float *cw, int n, uint8_t *bits)
    {
        CCSDSTurbo t((codings::turbo::turbo_base_t)base, (codings::turbo::turbo_rate_t)rate);
        const int len = t.codeword_length();
        std::vector<float> in(len);
        std::vector<uint8_t> fr(base);
        for (int f = 0; f < n; f++)
        {
            memcpy(in.data(), cw + (size_t)f * len, len * sizeof(float));
            t.decode(in.data(), fr.data(), iters);
            for (int i = 0; i < base * 8; i++)
                bits[(size_t)f * base * 8 + i] = (fr[i / 8] >> (7 - i % 8)) & 1;
        }
    }
    // the first iteration's two convcode_extrinsic calls on one prepared codeword: the two constituent streams, the a-priori arrays [2][L] after the upper pass,
    // what the lower pass receives (message_interleave of them) and what it leaves
    void turboref_bcjr(int rate, int base, const float *cw, double *stream0, double *stream1, double *after_upper, double *lower_in, double *after_lower)
    {
        CCSDSTurbo t((codings::turbo::turbo_base_t)base, (codings::turbo::turbo_rate_t)rate);
        std::vector<double> streams[2];
        split(t, cw, streams);
        memcpy(stream0, streams[0].data(), streams[0].size() * sizeof(double));
        memcpy(stream1, streams[1].data(), streams[1].size() * sizeof(double));
        const int L = base * 8;
        std::vector<double> m0(L, log(0.5)), m1(L, log(0.5));
        double *rows[2] = {m0.data(), m1.data()};
        double **messages = rows;
        const double nv = t.d_sigma * t.d_sigma;
        convcode_extrinsic(streams[0].data(), (double)streams[0].size(), &messages, t.d_turbo.upper_code, nv, 0);
        memcpy(after_upper, m0.data(), L * sizeof(double));
        memcpy(after_upper + L, m1.data(), L * sizeof(double));
        for (int i = 0; i < L; i++)
        {
            lower_in[i] = after_upper[t.d_pi[i]];
            lower_in[L + i] = after_upper[L + t.d_pi[i]];
        }
        memcpy(m0.data(), lower_in, L * sizeof(double));
        memcpy(m1.data(), lower_in + L, L * sizeof(double));
        convcode_extrinsic(streams[1].data(), (double)streams[1].size(), &messages, t.d_turbo.lower_code, nv, 0);
        memcpy(after_lower, m0.data(), L * sizeof(double));
        memcpy(after_lower + L, m1.data(), L * sizeof(double));
    }
    // turbo_decode's loop (libturbocodes.c:160-186) by hand over convcode_extrinsic, on one prepared codeword. The lower pass is asked for its decision in every
    // iteration (the decision reads the arrays and changes none), so bits[k - 1][L] is what turbo_decode returns for `iterations` = k, for every k <= iters.
    // rec[0], rec[1]: two iterations (1-based, 0 = none) whose passes are recorded to passes[x][4][2][L]: the a-priori arrays the upper pass receives and
    // leaves, and the ones the lower pass receives (interleaved) and leaves (before message_deinterleave). stream0 / stream1 (may be null): the two constituent
    // streams. perturb != 0: after every pass each message m becomes m + s * 2^-43 * max(1, |m|), s = +-1 from a generator seeded with `perturb`.
    void turboref_iterate(int rate, int base, const float *cw, int iters, uint8_t *bits, const int *rec, double *passes, double *stream0, double *stream1, uint64_t perturb)
    {
        CCSDSTurbo t((codings::turbo::turbo_base_t)base, (codings::turbo::turbo_rate_t)rate);
        std::vector<double> streams[2];
        split(t, cw, streams);
        if (stream0)
            memcpy(stream0, streams[0].data(), streams[0].size() * sizeof(double));
        if (stream1)
            memcpy(stream1, streams[1].data(), streams[1].size() * sizeof(double));
        const int L = base * 8;
        std::vector<double> m0(L, log(0.5)), m1(L, log(0.5));
        double *rows[2] = {m0.data(), m1.data()};
        double **messages = rows;
        const double nv = t.d_sigma * t.d_sigma;
        uint64_t x = perturb;
        auto shake = [&]() {
            if (!perturb)
                return;
            for (int r = 0; r < 2; r++)
                for (int i = 0; i < L; i++)
                {
                    x += 0x9E3779B97F4A7C15ull; // splitmix64
                    uint64_t z = x;
                    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
                    z ^= z >> 31;
                    const double m = rows[r][i];
                    rows[r][i] = m + ((z >> 63) ? 1.0 : -1.0) * ldexp(1.0, -43) * std::max(1.0, fabs(m));
                }
        };
        auto record = [&](int it, int which) {
            for (int k = 0; k < 2; k++)
                if (passes && rec && rec[k] == it + 1)
                {
                    double *p = passes + ((size_t)k * 4 + which) * 2 * L;
                    memcpy(p, m0.data(), L * sizeof(double));
                    memcpy(p + L, m1.data(), L * sizeof(double));
                }
        };
        for (int it = 0; it < iters; it++)
        {
            record(it, 0);
            free(convcode_extrinsic(streams[0].data(), (double)streams[0].size(), &messages, t.d_turbo.upper_code, nv, 0));
            record(it, 1);
            shake();
            message_interleave(&messages, t.d_turbo);
            record(it, 2);
            int *decoded = convcode_extrinsic(streams[1].data(), (double)streams[1].size(), &messages, t.d_turbo.lower_code, nv, 1);
            record(it, 3);
            for (int i = 0; i < L; i++) // turbo_deinterleave
                bits[(size_t)it * L + t.d_pi[i]] = decoded[i] ? 1 : 0;
            free(decoded);
            shake();
            message_deinterleave(&messages, t.d_turbo);
        }
    }
}
