// tools/fsk_golden_driver.cpp -- TEST INFRASTRUCTURE ONLY: the driver tools/gen_fsk_golden.py compiles (into a temporary directory, with the oracle's recorded
// flags -O2 -ffp-contract=off and ref_shim/) next to the reference's own block sources, to record what fsk_demod / sdpsk_demod compute as fixtures under
// tests/golden/fsk/. Nothing here is product code and nothing of it is committed in compiled form.
//
// The chain is built the way BaseDemodModule::initb (module_demod_base.cpp:59-208) and FSKDemodModule::init / SDPSKDemodModule::init
// (module_fsk_demod.cpp:59-84, module_sdpsk_demod.cpp:56-71) build it, from the reference's own block classes, and driven synchronously -- source buffer
// swapped in, every block's work() called in chain order -- which is arithmetically what the modules' thread-per-block topology computes (dsp::stream is a
// strict hand-off) without the threads' habit of dropping the stream's tail at stop(). Built with -fno-access-control so that work() can be called.
//
// Two members of MMClockRecoveryBlock<float> have no initialiser in the reference (`sample`, `last_sample`, clock_recovery_mm.h): pinned to zero here.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "logger.h"
std::shared_ptr<slog::Logger> logger = std::make_shared<slog::Logger>();

#include "common/dsp/block.h"
#include "common/dsp/clock_recovery/clock_recovery_mm.h"
#include "common/dsp/demod/quadrature_demod.h"
#include "common/dsp/filter/fir.h"
#include "common/dsp/filter/firdes.h"
#include "common/dsp/resamp/smart_resampler.h"
#include "common/dsp/utils/agc.h"
#include "common/dsp/utils/correct_iq.h"

#include "../include/sdhip.h" // the plain-C configuration structs

namespace
{
    template <class B>
    bool step(const std::shared_ptr<B> &b)
    { // a block whose predecessor handed nothing on (an empty resampler output) is not called: its read() would wait
        if (!b || !b->input_stream->getReady())
            return false;
        b->work();
        return true;
    }
    struct Tap
    {
        float *dst;
        int64_t cap, n = 0;
        void take(const float *src, int64_t cnt)
        {
            if (!dst)
                return;
            const int64_t k = std::max<int64_t>(0, std::min(cnt, cap - n));
            memcpy(dst + n, src, (size_t)k * sizeof(float));
            n += k;
        }
    };
}

extern "C"
{
    // iq: n complex floats. cuts: ascending sample positions at which a source buffer ends early, on top of the module's d_buffer_size grid (NULL / 0: none).
    // soft / syms: one int8 / one float per symbol (capacity cap). stage[s] (may be NULL), room for stage_cap SAMPLES each, the output of
    // 0 complex AGC (2 floats per sample) | 1 quadrature demodulator | 2 DC block | 3 float AGC (fsk) | 4 FIR | 5 clock recovery; stage_n[s] = floats recorded.
    // info[4] = {final_sps, final_samplerate, d_buffer_size, filter taps}. Returns the symbol count, < 0 on error.
    int64_t fskref_run(const sdhip_demod_cfg *c, const sdhip_fsk_ext *x, const float *iq, int64_t n, const int64_t *cuts, int ncuts, int8_t *soft, float *syms, int64_t cap,
                       float **stage, int64_t stage_cap, int64_t *stage_n, float *info)
    {
        // ---- BaseDemodModule ctor + initb
        const long d_samplerate = (long)c->samplerate;
        const int d_symbolrate = (int)c->symbolrate;
        int d_buffer_size = c->buffer_size > 0 ? c->buffer_size : std::min<int>(dsp::STREAM_BUFFER_SIZE, std::max<int>(8192 + 1, d_samplerate / 200));
        const float MIN_SPS = c->min_sps, MAX_SPS = c->max_sps;
        const float input_sps = (float)d_samplerate / (float)d_symbolrate;
        const bool resample = input_sps > MAX_SPS || input_sps < MIN_SPS;
        const int range = pow(10, (std::to_string(int(d_symbolrate)).size() - 1));
        float final_samplerate = d_samplerate;
        if (c->custom_samplerate > 0)
            final_samplerate = (long)c->custom_samplerate;
        else if (MAX_SPS == MIN_SPS)
            final_samplerate = d_symbolrate * MAX_SPS;
        else if (input_sps > MAX_SPS)
            final_samplerate = resample ? (round(d_symbolrate / range) * range) * MAX_SPS : d_samplerate;
        else if (input_sps < MIN_SPS)
            final_samplerate = resample ? d_symbolrate * MIN_SPS : d_samplerate;
        const float decimation_factor = d_samplerate / final_samplerate;
        if (resample)
            d_buffer_size *= ceil(decimation_factor);
        if (d_buffer_size > 8192 * 20)
            d_buffer_size = 8192 * 20;
        const float final_sps = final_samplerate / (float)d_symbolrate;
        if (c->freq_shift != 0 || c->doppler)
            return -2; // not part of the recorded cases

        auto in = std::make_shared<dsp::stream<complex_t>>();
        std::shared_ptr<dsp::stream<complex_t>> cur = in;
        std::shared_ptr<dsp::CorrectIQBlock<complex_t>> dc_blocker;
        std::shared_ptr<dsp::SmartResamplerBlock<complex_t>> rresamp;
        if (c->dc_block)
        {
            dc_blocker = std::make_shared<dsp::CorrectIQBlock<complex_t>>(cur);
            cur = dc_blocker->output_stream;
        }
        if (resample)
        {
            rresamp = std::make_shared<dsp::SmartResamplerBlock<complex_t>>(cur, final_samplerate, d_samplerate);
            cur = rresamp->output_stream;
        }
        auto agc = std::make_shared<dsp::AGCBlock<complex_t>>(cur, c->agc_rate, 1.0f, 1.0f, 65536);
        // ---- FSKDemodModule::init / SDPSKDemodModule::init
        auto qua = std::make_shared<dsp::QuadratureDemodBlock>(agc->output_stream, 1.0f);
        auto dcb2 = std::make_shared<dsp::CorrectIQBlock<float>>(qua->output_stream);
        std::shared_ptr<dsp::AGCBlock<float>> agc2;
        std::shared_ptr<dsp::stream<float>> fcur = dcb2->output_stream;
        if (x->kind == SDHIP_REAL_FSK)
        {
            agc2 = std::make_shared<dsp::AGCBlock<float>>(fcur, 0.1f, 0.5f, 1.0f, 65535.0f);
            fcur = agc2->output_stream;
        }
        std::vector<float> taps;
        if (x->kind == SDHIP_REAL_FSK && x->basic_shaping)
        {
            for (int i = 0; i < final_sps; i++)
                taps.push_back(0.1f);
        }
        else
            taps = dsp::firdes::root_raised_cosine(1, final_samplerate, d_symbolrate, c->rrc_alpha, c->rrc_taps);
        auto rrc = std::make_shared<dsp::FIRBlock<float>>(fcur, taps);
        auto rec = std::make_shared<dsp::MMClockRecoveryBlock<float>>(rrc->output_stream, final_sps, c->clock_gain_omega, c->clock_mu, c->clock_gain_mu,
                                                                      c->clock_omega_relative_limit);
        rec->sample = 0.0f;
        rec->last_sample = 0.0f;
        if (info)
        {
            info[0] = final_sps;
            info[1] = final_samplerate;
            info[2] = (float)d_buffer_size;
            info[3] = (float)taps.size();
        }
        Tap tap[6];
        for (int s = 0; s < 6; s++)
            tap[s] = Tap{stage ? stage[s] : nullptr, s == 0 ? 2 * stage_cap : stage_cap};
        const float scale = x->kind == SDHIP_REAL_FSK ? 50.0f : 400.0f;
        auto clampf = [](float v) -> int8_t { // module_demod_base.h:106-113
            if (v < -128.0)
                return -127;
            if (v > 127.0)
                return 127;
            return v;
        };
        int64_t nsym = 0, pos = 0;
        int ci = 0;
        while (pos < n)
        {
            int64_t end = std::min<int64_t>(n, pos + d_buffer_size);
            while (ci < ncuts && cuts[ci] <= pos)
                ci++;
            if (ci < ncuts && cuts[ci] < end)
                end = cuts[ci];
            const int m = (int)(end - pos);
            if (c->iq_swap)
                for (int i = 0; i < m; i++)
                    in->writeBuf[i] = complex_t(iq[2 * (pos + i) + 1], iq[2 * (pos + i)]);
            else
                memcpy(in->writeBuf, iq + 2 * pos, (size_t)m * sizeof(complex_t));
            in->swap(m);
            pos = end;
            step(dc_blocker);
            step(rresamp);
            if (step(agc))
                tap[0].take((const float *)agc->output_stream->readBuf, 2 * (int64_t)agc->output_stream->getDataSize());
            if (step(qua))
                tap[1].take(qua->output_stream->readBuf, qua->output_stream->getDataSize());
            if (step(dcb2))
                tap[2].take(dcb2->output_stream->readBuf, dcb2->output_stream->getDataSize());
            if (step(agc2))
                tap[3].take(agc2->output_stream->readBuf, agc2->output_stream->getDataSize());
            if (step(rrc))
                tap[4].take(rrc->output_stream->readBuf, rrc->output_stream->getDataSize());
            if (!step(rec))
                continue;
            const int dat_size = rec->output_stream->read();
            if (dat_size > 0)
            {
                const float *rb = rec->output_stream->readBuf;
                tap[5].take(rb, dat_size);
                for (int i = 0; i < dat_size; i++)
                {
                    if (nsym < cap)
                    {
                        syms[nsym] = rb[i];
                        soft[nsym] = clampf(rb[i] * scale); // module_fsk_demod.cpp:133-134, module_sdpsk_demod.cpp:119-120
                    }
                    nsym++;
                }
            }
            rec->output_stream->flush();
        }
        if (stage_n)
            for (int s = 0; s < 6; s++)
                stage_n[s] = tap[s].n;
        return nsym;
    }

    // MMClockRecoveryBlock<float>(omega, omegaGain, mu, muGain, omegaLimit) alone over n samples fed as one stream in STREAM-sized buffers: the symbols it emits
    int64_t fskref_mm(float omega, float gw, float mu, float gmu, float lim, const float *in_f, int64_t n, float *out, int64_t cap)
    {
        auto in = std::make_shared<dsp::stream<float>>();
        auto rec = std::make_shared<dsp::MMClockRecoveryBlock<float>>(in, omega, gw, mu, gmu, lim);
        rec->sample = 0.0f;
        rec->last_sample = 0.0f;
        int64_t no = 0;
        for (int64_t pos = 0; pos < n; pos += 65536)
        {
            const int m = (int)std::min<int64_t>(65536, n - pos);
            memcpy(in->writeBuf, in_f + pos, (size_t)m * sizeof(float));
            in->swap(m);
            rec->work();
            const int k = rec->output_stream->read();
            for (int i = 0; i < k && no < cap; i++)
                out[no++] = rec->output_stream->readBuf[i];
            rec->output_stream->flush();
        }
        return no;
    }
}
