// tools/ccsds_ldpc_golden_driver.cpp -- TEST INFRASTRUCTURE ONLY: the driver tools/gen_ccsds_ldpc_golden.py compiles (into a temporary directory, with the oracle's
// recorded flags -O2 -ffp-contract=off and ref_shim/) next to the reference's own sources, to record what ccsds_ldpc_decoder computes at "ldpc_rate": "7/8" as
// fixtures under tests/golden/ldpc/. Nothing here is product code and nothing of it is committed in compiled form.
//
// It restates CCSDSLDPCDecoderModule::process() (module_ccsds_ldpc_decoder.cpp:134-277) over an in-memory stream, on the reference's own CorrelatorGeneric,
// rotate_soft, derand_ccsds_soft, CCSDSLDPC and BPSK_CCSDS_Deframer. read_data() becomes a FIFO that the caller fills in pieces: a read that the FIFO cannot
// serve -- the main read of a frame, or the `pos` bytes behind a slide -- waits for the next piece, and the stream ends at the first incomplete read.
// get_best_ldpc_decoder() asks the event bus for the SIMD plugins' decoders; the target is the build without them, so it is defined here to hand out
// LDPCDecoderGeneric (simd() == 1). The module's ldpc_output_buffer is never initialised where the decoder does not write (bits 8158 / 8159 of a frame): zero here.
// Built with -fno-access-control (the correlator's tables are private) and -Dvolk_8i_s32f_convert_32f=volk_8i_s32f_convert_32f_u (the shim's name for VOLK's
// generic kernel).
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "logger.h"
std::shared_ptr<slog::Logger> logger = std::make_shared<slog::Logger>();

#include "common/codings/deframing/bpsk_ccsds_deframer.h"
#include "common/codings/generic_correlator.h"
#include "common/codings/ldpc/ccsds_ldpc.h"
#include "common/codings/ldpc/ldpc_decoder_generic.h"
#include "common/codings/randomization.h"
#include "common/codings/rotation.h"

namespace codings
{
    namespace ldpc
    {
        LDPCDecoder::LDPCDecoder(Sparse_matrix) {}
        LDPCDecoder::~LDPCDecoder() {}
        LDPCDecoder *get_best_ldpc_decoder(Sparse_matrix pcm) { return new LDPCDecoderGeneric(pcm); }
    }
}

namespace
{
    struct Desc
    {
        int64_t offset;
        int sync;
        float cor;
        int corrections;
        int locked;
    };
    int sync_index(dsp::constellation_type_t c, phase_t phase, bool swap)
    { // the inverse of generic_correlator.cpp:233-261
        if (c == dsp::BPSK)
            return phase == PHASE_180 ? 1 : 0;
        if (c == dsp::QPSK)
            return (int)phase;
        if (!swap)
            return phase == PHASE_90 ? 0 : 1;
        return phase == PHASE_0 ? 2 : 3;
    }
    struct Run
    {
        dsp::constellation_type_t d_constellation;
        bool d_derand, d_internal_stream;
        int d_ldpc_iterations, d_cadu_size, d_cadu_bytes;
        const int d_ldpc_asm_size = 32;
        int d_ldpc_frame_size, d_ldpc_codeword_size, d_ldpc_data_size;
        std::unique_ptr<codings::ldpc::CCSDSLDPC> ldpc_dec;
        std::unique_ptr<CorrelatorGeneric> correlator;
        std::unique_ptr<deframing::BPSK_CCSDS_Deframer> deframer;
        std::vector<int8_t> soft_buffer, ldpc_input_buffer;
        std::vector<uint8_t> ldpc_output_buffer, deframer_buffer;
        // the stream
        std::vector<int8_t> fifo;
        size_t rd = 0;
        int64_t stream_pos = 0; // stream position of the next byte read
        // a read in progress behind a slide
        bool sliding = false;
        int slide_pos = 0;
        int64_t read_start = 0;
        phase_t phase = PHASE_0;
        bool swap = false;
        // results
        float correlator_cor = 0;
        bool correlator_locked = false;
        int ldpc_corr = 0;
        std::vector<Desc> descs;
        std::vector<uint8_t> out;

        Run(int constellation, int derand, int iterations, int internal_stream, int cadu_size, uint32_t asm_sync)
            : d_constellation(constellation == 0 ? dsp::BPSK : (constellation == 2 ? dsp::QPSK : dsp::OQPSK)), d_derand(derand), d_internal_stream(internal_stream),
              d_ldpc_iterations(iterations), d_cadu_size(cadu_size), d_cadu_bytes((cadu_size + 7) / 8)
        {
            ldpc_dec = std::make_unique<codings::ldpc::CCSDSLDPC>(codings::ldpc::RATE_7_8, 0);
            d_ldpc_frame_size = ldpc_dec->frame_length() + d_ldpc_asm_size;
            d_ldpc_codeword_size = ldpc_dec->frame_length();
            d_ldpc_data_size = ldpc_dec->data_length();
            std::vector<uint8_t> syncword;
            for (int s = 31; s >= 0; s--)
                syncword.push_back((0x1acffc1du >> s) & 1);
            correlator = std::make_unique<CorrelatorGeneric>(d_constellation, syncword, d_ldpc_frame_size);
            if (d_internal_stream)
            {
                deframer = std::make_unique<deframing::BPSK_CCSDS_Deframer>(d_cadu_size, asm_sync);
            }
            soft_buffer.resize(d_ldpc_frame_size);
            ldpc_input_buffer.resize(d_ldpc_codeword_size);
            ldpc_output_buffer.assign(d_ldpc_codeword_size, 0);
            deframer_buffer.resize((size_t)d_ldpc_frame_size * 64);
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
                    if (!read_data(soft_buffer.data(), d_ldpc_frame_size))
                        return;
                    const int pos = correlator->correlate(soft_buffer.data(), phase, swap, correlator_cor, d_ldpc_frame_size);
                    correlator_locked = pos == 0;
                    if (pos != 0 && pos < d_ldpc_frame_size)
                    {
                        memmove(soft_buffer.data(), &soft_buffer[pos], d_ldpc_frame_size - pos);
                        sliding = true;
                        slide_pos = pos;
                    }
                }
                if (sliding)
                {
                    if (!read_data(&soft_buffer[d_ldpc_frame_size - slide_pos], slide_pos))
                        return;
                    sliding = false;
                }
                else
                    slide_pos = 0;
                const int64_t offset = read_start + slide_pos;
                slide_pos = 0;
                if (d_constellation == dsp::OQPSK)
                {
                    rotate_soft(soft_buffer.data(), d_ldpc_frame_size, phase, false);
                    if (swap)
                    {
                        int8_t last_q_oqpsk = 0;
                        for (int i = (d_ldpc_frame_size / 2) - 1; i >= 0; i--)
                        {
                            int8_t back = soft_buffer[i * 2 + 1];
                            soft_buffer[i * 2 + 1] = last_q_oqpsk;
                            last_q_oqpsk = back;
                        }
                    }
                }
                else
                    rotate_soft(soft_buffer.data(), d_ldpc_frame_size, phase, swap);
                if (d_derand)
                    derand_ccsds_soft(&soft_buffer[d_ldpc_asm_size], d_ldpc_codeword_size);
                memcpy(ldpc_input_buffer.data(), &soft_buffer[d_ldpc_asm_size], d_ldpc_codeword_size);
                ldpc_corr = ldpc_dec->decode(ldpc_input_buffer.data(), ldpc_output_buffer.data(), d_ldpc_iterations);
                descs.push_back(Desc{offset, sync_index(d_constellation, phase, swap), correlator_cor, ldpc_corr, correlator_locked ? 1 : 0});
                if (d_internal_stream)
                {
                    const int frames = deframer->work(ldpc_output_buffer.data(), d_ldpc_data_size, deframer_buffer.data());
                    for (int i = 0; i < frames; i++)
                        out.insert(out.end(), &deframer_buffer[(size_t)i * d_cadu_bytes], &deframer_buffer[(size_t)(i + 1) * d_cadu_bytes]);
                }
                else
                {
                    for (int i = 0; i < d_ldpc_codeword_size; i++)
                        deframer_buffer[i / 8] = deframer_buffer[i / 8] << 1 | ldpc_output_buffer[i];
                    const uint32_t sync = 0x1acffc1d;
                    const uint8_t *sp = (const uint8_t *)&sync;
                    out.insert(out.end(), sp, sp + 4);
                    out.insert(out.end(), deframer_buffer.begin(), deframer_buffer.begin() + (d_ldpc_frame_size - d_ldpc_asm_size) / 8);
                }
            }
        }
    };
}

extern "C"
{
    void *ldpcref_create(int constellation, int derand, int iterations, int internal_stream, int cadu_size, uint32_t asm_sync)
    {
        return new Run(constellation, derand, iterations, internal_stream, cadu_size, asm_sync);
    }
    void ldpcref_destroy(void *h) { delete (Run *)h; }
    void ldpcref_feed(void *h, const int8_t *soft, int64_t n) { ((Run *)h)->feed(soft, n); }
    int64_t ldpcref_ndesc(void *h) { return (int64_t)((Run *)h)->descs.size(); }
    int64_t ldpcref_nout(void *h) { return (int64_t)((Run *)h)->out.size(); }
    // offsets[n], sync[n], cor[n], corrections[n], locked[n]; out bytes; stats4 = {correlator_lock, ldpc_corr, deframer state, 0}, cor1 = correlator_corr
    void ldpcref_results(void *h, int64_t *offsets, int *sync, float *cor, int *corrections, int *locked, uint8_t *out, int *stats4, float *cor1)
    {
        Run *r = (Run *)h;
        for (size_t i = 0; i < r->descs.size(); i++)
        {
            offsets[i] = r->descs[i].offset;
            sync[i] = r->descs[i].sync;
            cor[i] = r->descs[i].cor;
            corrections[i] = r->descs[i].corrections;
            locked[i] = r->descs[i].locked;
        }
        memcpy(out, r->out.data(), r->out.size());
        stats4[0] = r->correlator_locked ? 1 : 0;
        stats4[1] = r->ldpc_corr;
        stats4[2] = r->deframer ? r->deframer->getState() : 0;
        stats4[3] = 0;
        *cor1 = r->correlator_cor;
    }
    // the correlator's tables: out = 4 x 32 floats. Returns their number.
    int ldpcref_syncwords(void *h, float *out)
    {
        Run *r = (Run *)h;
        for (size_t s = 0; s < r->correlator->syncwords.size(); s++)
            memcpy(out + 32 * s, r->correlator->syncwords[s].data(), 32 * sizeof(float));
        return (int)r->correlator->syncwords.size();
    }
    // CorrelatorGeneric::correlate on a window of 33 bytes at every position p < n - 32: the one position it then looks at is p
    void ldpcref_positions(void *h, const int8_t *soft, int64_t n, float *cor, uint8_t *sync)
    {
        Run *r = (Run *)h;
        int8_t win[33];
        for (int64_t p = 0; p + 33 <= n; p++)
        {
            memcpy(win, soft + p, 33);
            phase_t ph = PHASE_0;
            bool sw = false;
            float c = 0;
            r->correlator->correlate(win, ph, sw, c, 33);
            cor[p] = c;
            sync[p] = (uint8_t)sync_index(r->d_constellation, ph, sw);
        }
    }
    // LDPCDecoderGeneric on ANY row list: rows[ncn][32] column indices (0xFFFF = no edge), n words of nvn soft bytes -> bits (nvn a word) and what decode returns
    void ldpcref_generic(const uint16_t *rows, int ncn, int nvn, const int8_t *in, int n, int iterations, uint8_t *bits, int *corrections)
    {
        codings::ldpc::Sparse_matrix pcm(ncn, nvn);
        for (int r = 0; r < ncn; r++)
            for (int k = 0; k < 32; k++)
                if (rows[r * 32 + k] != 0xFFFF)
                    pcm.add_connection(r, rows[r * 32 + k]);
        codings::ldpc::LDPCDecoderGeneric dec(pcm);
        for (int f = 0; f < n; f++)
            corrections[f] = dec.decode(bits + (size_t)f * nvn, in + (size_t)f * nvn, iterations);
    }
    // CCSDSLDPC::decode over LDPCDecoderGeneric on n prepared codewords of 8160 soft bytes: bits (8160 a frame, the last two 0) and what decode returns
    void ldpcref_unit(const int8_t *cw, int n, int iterations, uint8_t *bits, int *corrections)
    {
        codings::ldpc::CCSDSLDPC dec(codings::ldpc::RATE_7_8, 0);
        std::vector<int8_t> in(8160);
        for (int f = 0; f < n; f++)
        {
            memcpy(in.data(), cw + (size_t)f * 8160, 8160);
            memset(bits + (size_t)f * 8160, 0, 8160);
            corrections[f] = dec.decode(in.data(), bits + (size_t)f * 8160, iterations);
        }
    }
}
