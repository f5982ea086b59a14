// The generation switch: which of the four one-wave-per-SIMD kernels (kernels_cw4 / wg4 / pf4 / pw4.hip) may serve a launch.  All are on by default;
// PROBAV_GEN1 in the environment (read once, on first use) or w4_set_enabled() sends an operator back to its general form for A/B runs.
// No HIP include: the parser and the mask test are pure (tests/test_w4_switch.py compiles them with the host compiler alone).
#pragma once
#include <cstring>

namespace probav {

enum class W4 { conv = 0, wgrad = 1, pw_fwd = 2, pw_bwd = 3 };     // conv3_w4 (C), conv3_wgrad_w4 (W), pw_fwd_w4 (F), pw_bwd_w4 (B)
constexpr unsigned w4_bit(W4 k) { return 1u << (int)k; }
inline bool w4_mask_enabled(unsigned disabled, W4 k) { return (disabled & w4_bit(k)) == 0; }

// PROBAV_GEN1 -> mask of disabled kernels.  THE grammar: the value is matched by PREFIX, the first matching row decides
inline unsigned w4_parse_disabled(const char* env)
{
    constexpr unsigned C = w4_bit(W4::conv), W = w4_bit(W4::wgrad), F = w4_bit(W4::pw_fwd), B = w4_bit(W4::pw_bwd);
    static const struct { const char* prefix; unsigned off; } rows[] = {
        {"1", C | W | F | B},       // "1", "1conv"
        {"c", C},                   // "conv", "c"
        {"w", W},                   // "wg", "w"
        {"pwf", F},                 // "pwf"
        {"pwb", B},                 // "pwb"
        {"pw", F | B},              // "pw", "pwx"
    };                              // unset, "", "0", "x", "p": none
    if (env) for (const auto& r : rows) if (strncmp(env, r.prefix, strlen(r.prefix)) == 0) return r.off;
    return 0;
}

bool w4_enabled(W4 k);                 // (kernels_x6.hip)
void w4_set_enabled(W4 k, int on);     // overrides the environment for this kernel

}  // namespace probav
