// encodings.cpp -- host-side encoding math of the DlQuantization analyzers.
//
// These are O(512) computations per channel on statistics already reduced on the device
// (stats.hip). They reproduce the reference arithmetic exactly, including its float/double
// mix (the analyzers are instantiated with DTYPE = float) and libstdc++'s std::min/std::max
// tie rules; the file is compiled with -ffp-contract=off like the reference (x86-64, no FMA).
//
//   getComputedEncodings           quantization_utils.cpp:58-143
//   gateMinMax / fillEncodingInfo  quantization_utils.cpp:145-156, TensorQuantizationSim.cpp:62-92
//   partial encodings              quantization_utils.cpp:158-228, TensorQuantizer.cpp:323-341
//   TF                             TfEncodingAnalyzer.cpp:80-101
//   TF-Enhanced                    TfEnhancedEncodingAnalyzer.cpp:78-392
//   Percentile                     PercentileEncodingAnalyzer.cpp:78-190, math_functions.cpp:404-439
//   MSE                            MseEncodingAnalyzer.cpp:79-264
//   Entropy                        EntropyEncodingAnalyzer.cpp:97-435, math_functions.cpp:562-641
#include "encodings.hpp"
#include "entropy_core.hpp"
#include "entropy_kl.hpp"
#include "mse_core.hpp"
#include "tfe_core.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <limits>
#include <numeric>
#include <utility>

namespace aimet_amd
{

namespace
{
constexpr double kGateEps  = 1e-5;   // quantization_utils.hpp:51 EPSILON
constexpr double kMinRange = 0.01;   // TfEncodingAnalyzer.h:81 / TfEnhancedEncodingAnalyzer.h:105

inline double sq(double v)
{
    return v * v;   // std::pow(v, 2) folds to v*v in the reference build (-O3)
}

aimet_tf_encoding make_enc(double mn, double mx, double d, double o, int32_t bw)
{
    aimet_tf_encoding e;
    e.min    = mn;
    e.max    = mx;
    e.delta  = d;
    e.offset = o;
    e.bw     = bw;
    return e;
}

}   // namespace

aimet_tf_encoding computed_encoding(int32_t bw, double mn, double mx, bool sym, bool strict, bool unsign)
{
    return mse::computed_encoding(bw, mn, mx, sym, strict, unsign);   // shared with the device (mse_core.hpp)
}

void gate_min_max(double& mn, double& mx)
{
    mn = std::min(mn, 0.0);
    mx = std::max(mx, 0.0);
    mx = std::max(mx, mn + kGateEps);
}

aimet_tf_encoding fill_encoding_info(int32_t bw, double mn, double mx)
{
    gate_min_max(mn, mx);
    double steps = std::pow(2.0, (uint8_t) bw) - 1;
    if (mn == -mx)
        steps -= 1;   // strict symmetric: 2^bw - 2 steps
    double delta  = (mx - mn) / steps;
    double offset = std::round(mn / delta);
    double lo     = offset * delta;
    return make_enc(lo, delta * steps + lo, delta, offset, (uint8_t) bw);
}

bool partial_encoding(int32_t bw, aimet_tf_encoding& e, bool sym, bool unsign, bool strict, std::string& err)
{
    if (e.min == 0 && e.max == 0)
    {
        // computeMinMaxRangeFromDeltaOffset
        if (e.bw == 0)
            return err = "Encodings must have a valid non-zero bitwidth", false;
        if (e.delta == 0 && e.offset > 0)
            return err = "Encoding must have a valid non-zero delta/offset if min and max are zero", false;
        double steps = std::pow(2.0, (uint8_t) bw) - 1;
        if (sym && strict)
            steps -= 1;
        e.min = e.offset * e.delta;
        if (sym && (e.min < 0.0 || !unsign))
            e.max = e.delta * std::floor(steps / 2);
        else
            e.max = e.delta * steps + e.min;
        if (e.max - e.min < kGateEps)
            gate_min_max(e.min, e.max);
        return true;
    }
    if (e.delta == 0)
    {
        // computeDeltaAndOffsetFromMinMax
        if (e.bw == 0)
            return err = "Encodings must have a valid non-zero bitwidth", false;
        if (e.delta != 0 && e.offset != 0)
            return err = "Encoding delta and offset must be zero to use this function", false;
        double mn = e.min, mx = e.max;
        e         = computed_encoding((uint8_t) bw, mn, mx, sym, strict, unsign);
        e.min     = mn;
        e.max     = mx;
        return true;
    }
    err = "Cannot determine how to compute partial encoding";
    return false;
}

void per_channel_table_host(const aimet_tf_encoding* encs, int64_t C, float* table)
{
    // AimetTensorQuantizer.cpp:262-299 executed as float32 torch ops on the CPU:
    // minimum/maximum propagate NaN, scalars are rounded to float, at::round is half-to-even.
    auto tmin = [](float a, float b) { return (std::isnan(a) || std::isnan(b)) ? NAN : (a < b ? a : b); };
    auto tmax = [](float a, float b) { return (std::isnan(a) || std::isnan(b)) ? NAN : (a > b ? a : b); };
    double steps = std::pow(2.0, encs[0].bw) - 1;
    if (encs[0].min == -encs[0].max)
        steps -= 1;
    const float fsteps = (float) steps;
    const float eps    = (float) 1e-5;
    for (int64_t c = 0; c < C; ++c)
    {
        float mn = tmin((float) encs[c].min, 0.0f);
        float mx = tmax((float) encs[c].max, 0.0f);
        mx       = tmax(mx, mn + eps);
        float d  = (mx - mn) / fsteps;
        table[c]         = mn;
        table[C + c]     = mx;
        table[2 * C + c] = d;
        table[3 * C + c] = std::nearbyint(mn / d);
    }
}

// ---------------------------------------------------------------------------------------------
// Histogram analyzers. `HistView` is the reconstructed PDF of one channel:
// xLeft[i] = (double)hist_min + (double)i * bucket_size (InitializePdf, signed branch).
// ---------------------------------------------------------------------------------------------
namespace
{

struct HistView
{
    float hist_min;
    double bucket;
    const double* pdf;
    double xl(int i) const
    {
        return (double) hist_min + (double) i * bucket;
    }
};

// findOriginalRange<float> (== TfEnhanced::_findRangeOfAggregateStats)
std::pair<float, float> observed_range(const HistView& h)
{
    float lo = (float) h.xl(0), hi = (float) h.xl(kPdfSize - 1);
    int first = -1, last = -1;
    for (int i = 0; i < kPdfSize; ++i)
        if (h.pdf[i] > 0)
        {
            first = i;
            break;
        }
    for (int i = kPdfSize - 1; i > 0; --i)
        if (h.pdf[i] > 0)
        {
            last = i;
            break;
        }
    if (first >= 0)
        lo = (float) h.xl(first);
    if (last >= 0)
        hi = (float) h.xl(last);
    lo = std::min(lo, 0.0f);
    hi = std::max(hi, 0.0f);
    hi = std::max(hi, lo + (float) kMinRange);
    return {lo, hi};
}

aimet_tf_encoding unseen_or_zero(bool stats_updated, int32_t bw, float steps)
{
    // "we have seen all zero data": a [-1, 1] encoding (TfEnhancedEncodingAnalyzer.cpp:86-99)
    if (!stats_updated)
        return make_enc(0, 0, 0, 0, 0);
    int isteps   = (int) steps;
    double delta = (1.0 - (-1.0)) / isteps;
    double off   = std::floor(-1.0 / delta);
    double lo    = off * delta;
    return make_enc(lo, lo + isteps * delta, delta, off, bw);
}

// ---- TF-Enhanced (tfe_core.hpp: shared with the device search in tfe_search.hip) ---------
aimet_tf_encoding tfe_encoding(const HistView& h, int32_t bw, bool sym, bool strict, bool unsign)
{
    int first = -1, last = -1;
    for (int i = 0; i < kPdfSize; ++i)
        if (h.pdf[i] > 0)
        {
            first = i;
            break;
        }
    for (int i = kPdfSize - 1; i > 0; --i)
        if (h.pdf[i] > 0)
        {
            last = i;
            break;
        }
    tfe::Hist th {h.hist_min, h.bucket, h.pdf};
    float lo, hi;
    tfe::observed_range(th, first, last, lo, hi);
    tfe::Setup st = tfe::setup(lo, hi, bw, sym, strict, unsign);
    float fseq[tfe::kSymF + 8];
    if (sym)
        tfe::fseq_sym(fseq);
    else
        tfe::fseq_asym(fseq);
    // the per-channel bin tables every candidate shares (tfe_core.hpp, as the device builds them)
    float cf[tfe::kBins];
    double pdf_c[tfe::kBins], cd_c[tfe::kBins];
    float cf_c[tfe::kBins];
    short pos[tfe::kBins];
    const float start = tfe::bins_start(th);
    const double step = tfe::bins_step(th);
    const bool skip   = tfe::bins_skip_empty(th);
    int nnz           = 0;
    for (int i = 0; i < tfe::kBins; ++i)
    {
        const double cd = tfe::bin_centre(start, step, i);
        cf[i]           = (float) cd;
        pos[i]          = (short) nnz;
        if (h.pdf[i] > 0 || !skip)
        {
            pdf_c[nnz] = h.pdf[i];
            cd_c[nnz]  = cd;
            cf_c[nnz]  = cf[i];
            ++nnz;
        }
    }
    const tfe::Bins B {start, step, cf, pdf_c, cd_c, cf_c, pos, nnz};
    float bestDelta = -1;
    int bestOffset  = -1;
    double best     = std::numeric_limits<double>::max();
    for (int t = 0; t < st.ncand; ++t)
    {
        float d;
        int o;
        if (!tfe::candidate(st, fseq, t, d, o))
            continue;
        double c = sym ? tfe::cost<true>(B, bw, d, o) : tfe::cost<false>(B, bw, d, o);
        if (c < best)
        {
            best       = c;
            bestDelta  = d;
            bestOffset = o;
        }
    }
    tfe::Result r = tfe::finish(st, bestDelta, bestOffset);
    return make_enc(r.min, r.max, r.delta, r.offset, bw);
}

// ---- Percentile ---------------------------------------------------------------------------
std::pair<float, float> percentile_range(const HistView& h, float percentile)
{
    auto range = observed_range(h);
    if (percentile == 100.0f)
        return range;
    const float width = (float) (h.xl(1) - h.xl(0));
    float pLo         = (float) h.xl(0);
    float pHi         = (float) h.xl(kPdfSize - 1) + width;
    double cdf[kPdfSize];
    std::partial_sum(h.pdf, h.pdf + kPdfSize, cdf);
    const float left = 1 - percentile / 100;
    for (int i = 0; i < kPdfSize; ++i)
        if (cdf[i] >= left)
        {
            pLo = (float) h.xl(i);
            break;
        }
    const float right = percentile / 100;
    for (int i = kPdfSize - 1; i >= 0; --i)
        if (cdf[i] < right && h.xl(i) < range.second)
        {
            pHi = (float) (h.xl(i) + width);
            break;
        }
    if (pLo == pHi)
        pHi += width;
    return {pLo, pHi};
}

// ---- MSE (mse_core.hpp: shared with the device search in mse_search.hip) -------------------
std::pair<float, float> mse_range(const HistView& h, int32_t bw, bool sym, bool strict, bool unsign)
{
    tfe::Hist th {h.hist_min, h.bucket, h.pdf};
    int first, last;
    tfe::first_last(h.pdf, first, last);
    float mins[mse::kMaxEdges + 1], maxs[mse::kMaxEdges + 1], cv[mse::kMaxEdges], cw[mse::kMaxEdges];
    mse::Setup st = mse::setup(th, first, last, mins, maxs, cv, cw);
    float bestErr = std::numeric_limits<float>::max();
    std::pair<float, float> best(st.lo, st.hi);
    for (long long t = 0; t < st.total; ++t)
    {
        float cLo, cHi;
        mse::candidate(st, mins, maxs, t, cLo, cHi);
        float err = mse::cost(bw, cv, cw, st.nc, cLo, cHi, sym, strict, unsign);
        if (err < bestErr)
        {
            bestErr = err;
            best    = {cLo, cHi};
        }
    }
    return best;
}

// ---- Entropy: KL-divergence range search over the TensorProfilingParams histogram -------------
// _optimizeKL (EntropyEncodingAnalyzer.cpp:226-435) with the arithmetic of entropy_kl.hpp (shared
// with the device search, entropy_search.hip) and glibc's log, which is what decides near-ties.
double glibc_log(double v)
{
    return std::log(v);
}

std::pair<float, float> kl_range(double tmin, double tmax, const double* tpp_hist, int32_t bw, bool sym, bool strict,
                                 bool unsign)
{
    double hist[kPdfSize];
    double lo, hi;
    entropy::kl_histogram(tmin, tmax, tpp_hist, sym, unsign, hist, lo, hi);
    if (bw != 8)
        return {(float) lo, (float) hi};
    const double w = (hi - lo) / (double) kPdfSize;
    short wa[entropy::kWindows], wb[entropy::kWindows];
    const int n   = entropy::windows(hist, lo, w, sym || strict, wa, wb);
    double left[kPdfSize];
    int zeros[kPdfSize + 1];
    entropy::Prefix pre {left, zeros, false};
    entropy::build_prefix(hist, left, zeros, pre.q_zero_rule);
    double best   = std::numeric_limits<double>::infinity();
    double bestLo = lo, bestHi = hi;
    for (int k = 0; k < n; ++k)
    {
        const entropy::WindowKl r = entropy::window_kl(hist, wa[k], wb[k], glibc_log, &pre);
        if (r.brk)
            break;
        if (r.dv < best)
        {
            best   = r.dv;
            bestLo = lo + (double) wa[k] * w;
            bestHi = lo + (double) (wb[k] + 1) * w;
        }
    }
    return {(float) bestLo, (float) bestHi};
}

}   // namespace

aimet_tf_encoding entropy_encoding(bool has_hist, bool stats_updated, double tmin, double tmax, const double* hist,
                                   int32_t bw, bool sym, bool strict, bool unsign)
{
    float steps = (float) (std::pow(2.0, bw) - 1);
    if (sym && strict)
        steps -= 1;
    if (!has_hist)
        return unseen_or_zero(stats_updated, bw, steps);
    std::pair<float, float> r = kl_range(tmin, tmax, hist, bw, sym, strict, unsign);
    return entropy_encoding_from_range(r.first, r.second, bw, sym, strict, unsign);
}

aimet_tf_encoding entropy_encoding_from_range(float kl_lo, float kl_hi, int32_t bw, bool sym, bool strict, bool unsign)
{
    float lo = std::min(kl_lo, 0.0f);
    float hi = std::max(kl_hi, 0.0f);
    return computed_encoding(bw, lo, hi, sym, strict, unsign);
}

aimet_tf_encoding tf_encoding(double accMin, double accMax, int32_t bw, bool sym, bool strict, bool unsign)
{
    return mse::tf_encoding(accMin, accMax, bw, sym, strict, unsign);   // shared with the device (blockwise.hip)
}

aimet_tf_encoding histogram_encoding(int scheme, bool initialized, bool stats_updated, float hist_min,
                                     double bucket_size, const double* pdf, float percentile, int32_t bw, bool sym,
                                     bool strict, bool unsign)
{
    float steps = (float) (std::pow(2.0, bw) - 1);
    if (scheme != AIMET_QUANTIZATION_TF_ENHANCED && sym && strict)
        steps -= 1;   // percentile / MSE reduce before the zero-data check
    if (!initialized)
        return unseen_or_zero(stats_updated, bw, steps);
    HistView h {hist_min, bucket_size, pdf};
    if (scheme == AIMET_QUANTIZATION_TF_ENHANCED)
        return tfe_encoding(h, bw, sym, strict, unsign);
    std::pair<float, float> r = scheme == AIMET_QUANTIZATION_PERCENTILE ? percentile_range(h, percentile)
                                                                         : mse_range(h, bw, sym, strict, unsign);
    float lo = std::min(r.first, 0.0f);
    float hi = std::max(r.second, 0.0f);
    return computed_encoding(bw, lo, hi, sym, strict, unsign);
}

void histogram_xleft(float hist_min, double bucket_size, double* xleft)
{
    HistView h {hist_min, bucket_size, nullptr};
    for (int i = 0; i < kPdfSize; ++i)
        xleft[i] = h.xl(i);
}

}   // namespace aimet_amd
