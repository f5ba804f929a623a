// Host helpers shared by the two spectral plans (adf_istft.hip, adf_stft.hip): both take an adf_istft_config and a host window, refuse the same
// geometries with the same words, and pin their work to the device their plan was created on.
#pragma once
#include "adf_api_internal.h"
#include "adf_istft.h"

#include <cmath>
#include <string>
#include <vector>

namespace adf_spectral {

inline int fail(const std::string& m) { adf_api::g_create_error = m; return 1; }

// The window in double: the caller's n_fft floats, or the periodic Hann window.
inline std::vector<double> window_f64(const adf_istft_config& c, const float* window) {
    std::vector<double> w(c.n_fft);
    for (int m = 0; m < c.n_fft; ++m) w[m] = window ? (double)window[m] : 0.5 - 0.5 * std::cos(2.0 * M_PI * m / c.n_fft);
    return w;
}

// The checks both directions share; `center_why` ends the sentence that refuses center = 0.
inline int check_config(const char* fn, const adf_istft_config* cfg, const char* center_why) {
    const std::string f = std::string(fn) + ": ";
    if (!cfg) return fail(f + "null config");
    const adf_istft_config& c = *cfg;
    if (c.n_fft < 32 || c.n_fft > 1024 || c.n_fft % 2) return fail(f + "n_fft must be even and in [32, 1024], got " + std::to_string(c.n_fft));
    if (c.hop_length < 32 || c.hop_length > 256 || c.hop_length % 32)
        return fail(f + "hop_length must be a multiple of 32 in [32, 256], got " + std::to_string(c.hop_length));
    if ((c.n_fft + c.hop_length - 1) / c.hop_length > adf::kIstftMaxD)
        return fail(f + "hop_length " + std::to_string(c.hop_length) + " is too small for n_fft " + std::to_string(c.n_fft) + ": ceil(n_fft / hop_length) must be at most 8");
    if (!c.center) return fail(f + "center must be true (" + center_why + ")");
    if (!(c.spec_abs_exponent > 0.0) || !std::isfinite(c.spec_abs_exponent)) return fail(f + "spec_abs_exponent must be > 0");
    if (!(c.spec_factor > 0.0) || !std::isfinite(c.spec_factor)) return fail(f + "spec_factor must be > 0");
    return 0;
}

struct DeviceScope {
    int prev = -1;
    bool ok = true;
    explicit DeviceScope(int device) {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) { ok = false; return; }
        if (cur != device) {
            if (hipSetDevice(device) != hipSuccess) { ok = false; return; }
            prev = cur;
        }
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

}  // namespace adf_spectral
