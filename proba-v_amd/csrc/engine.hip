// Engine: sequences the HIP kernels into the WDSR-B Conv3D network of models/modelsTF.py:15-203
// (forward) and its reverse-mode gradient (what tf.GradientTape computes at models/trainClass.py:126-131),
// and exports the C ABI of include/probav_hip.h.  Host-side C++ only decides shapes, offsets and launch
// order; it never touches tensor data and never synchronises.
#include "probav_common.h"
#include "../../include/probav_hip.h"
#include <stdio.h>
#include <string.h>
#include <array>
#include <string>
#include <vector>

using namespace probav;

#include "kernels_mfma.h"
#include "kernels_x6.h"
#include "kernels_gemm.h"
#include "kernels_gemm_pw.h"
#include "kernels_gemm_x6.h"

// MFMA operand fragments: offsets into the workspace's wpack region (-1 = none)
struct ConvFrags { long f32 = -1, x6 = -1, h3 = -1, h3t = -1; };   // one direction of a 3x3x3 layer; h3t: per-tap H3 fragments of a 25-channel layer
struct PwFrags { long w1 = -1, w2 = -1, w2b = -1, w1c = -1; };     // one arithmetic of a block's fused pointwise pair: W1, W2 (forward), W2, W1 (backward's operands)

struct LayerRec {
    char name[32];
    WnLayer wn;
    int kh, kw, kt;
    ConvFrags pk[2];          // forward, backward-data
};

// what a kernel family (probav_engine_set_impl) may use: 0 direct kernels, 1 MFMA row-tile kernels, 2 MFMA + strip convolution where it
// applies, 3 = 2 with the x6 kernels (fp32 products as six bf16-piece MFMA products) where they exist, 4 = 3 with the H3 arithmetic (three
// products of scaled fp16 piece pairs) where it exists
enum class PairKind { none = 0, tuned = 1, gemm = 2 };      // un-fused | the tuned pair of the shipped shape (kernels_mfma / kernels_x6) | the general matrix route's (kernels_gemm_pw.hip)
struct Family {
    bool mfma;                // MFMA kernels, and the dedicated small kernels (upscale layer, one-channel input, fused residual path, tuned direct backward-filter)
    bool strip;               // MFMA strip convolution
    bool x6;                  // split-operand kernels
    int arith;                // their arithmetic: 0 none, 1 X6, 2 H3
    PairKind pw_fused;        // the fused pointwise pair (expConv + ReLU + decConv in one launch each way): which kernels run it, if any
    bool gemm;                // the general matrix route (kernels_gemm.hip) wherever a launch would otherwise fall to the generic direct kernels
    int gemm_arith;           // the arithmetic of the route's convolution launches (forward, backward-data): 0 fp32 (kernels_gemm.hip), 1 X6 (kernels_gemm_x6.hip)
    bool gemm_exotic;         // the route also takes the launches conv_route / wgrad_route call exotic (the 19-frame reducer's), on the wide predicates of kernels_gemm.h
};
// gemm: the engine's switch (probav_engine_set_gemm_route), kept on the engine apart from the family and folded in here, so that a change of family keeps it;
// it needs the matrix kernels' family (impl >= 1): family 0 stays the direct kernels everywhere.  pair_gemm: the second switch (probav_engine_set_gemm_pair) on a block
// geometry that gemm_pw_supported takes; it fuses the pair only on the route, and only where the tuned pair does not exist.  gemm_x6: the third switch
// (probav_engine_set_gemm_x6): the route's convolution launches in x6 arithmetic; it changes nothing but those launches' kernel.  gemm_exotic: the fourth switch
// (probav_engine_set_gemm_exotic): the exotic geometries, which return to the direct kernel before the route is asked, go to the route instead; only a 19-frame network has any
static Family make_family(int impl, bool pw_mfma, bool gemm = false, bool pair_gemm = false, bool gemm_x6 = false, bool gemm_exotic = false)
{
    Family f;
    f.mfma = impl >= 1; f.strip = impl >= 2; f.x6 = impl >= 3; f.arith = impl >= 4 ? 2 : (impl >= 3 ? 1 : 0);
    f.gemm = f.mfma && gemm;
    f.gemm_arith = f.gemm && gemm_x6 ? 1 : 0;
    f.gemm_exotic = f.gemm && gemm_exotic;
    f.pw_fused = !f.mfma ? PairKind::none : (pw_mfma ? PairKind::tuned : (f.gemm && pair_gemm ? PairKind::gemm : PairKind::none));
    return f;
}

struct probav_engine {
    probav_net_cfg cfg;
    std::vector<LayerRec> layers;
    int64_t nparams = 0, weff_count = 0, cout_total = 0, cin_total = 0;
    WnLayer* d_layers = nullptr;
    Family fam = {};
    int impl = 4;                                   // what fam was made from (probav_engine_set_impl)
    bool gemm = false;                              // probav_engine_set_gemm_route: folded into fam by make_family
    bool gemm_pair = false;                         // probav_engine_set_gemm_pair: the wish; folded into fam (with pw_gemm) by make_family
    bool gemm_x6 = false;                           // probav_engine_set_gemm_x6: the wish; folded into fam (with gemm) by make_family
    bool gemm_exotic = false;                       // probav_engine_set_gemm_exotic: the wish; folded into fam (with gemm) by make_family
    bool pw_gemm = false;                           // the block geometry has a general fused pointwise pair (gemm_pw_supported)
    int32_t launched[4] = {0, 0, 0, 0};             // what conv_fwd / conv_wgrad have launched, as probav_engine_route_counts counts (probav_engine_launched_counts)
    int iMain = -1, iResid1 = -1, iResid2 = -1, iResid3 = -1, iUp = -1;
    std::vector<int> iExp, iDec, iNorm, iRed;
    ReduceSide side = {};                           // side stream of the slab sums (probav_common.h), created on first use
    int side_mode = 2;                              // probav_engine_side_stream(): 0 off, 1 small work only, 2 + the backward-filter kernels
    bool side_tried = false;
    struct RedSpec { int k, p, pt, refl, refl_t; };   // one valid convReducer: kernel size, H/W pad, depth pad, mirrored H/W pad, mirrored depth pad
    std::vector<RedSpec> redSpec;
    int Hin = 0;
    // MFMA operand fragments: one packing job per (layer or block, use, arithmetic); their offsets live in LayerRec::pk and pkBlk
    std::vector<PackJob> jobs;
    PackJob* d_jobs = nullptr;
    int64_t wpack_count = 0;
    std::vector<std::array<PwFrags, 3>> pkBlk;   // per residual block, per arithmetic (fp32, X6, H3)
    bool pw_mfma = false;     // the block geometry has a fused pointwise pair
    bool fwd_amax = false;    // the last training forward filled the amax slots of the saved activations (H3 kernels, impl 4)
    PairKind fwd_pair = PairKind::none; // ... and ran the pointwise pair in this form, with this workspace layout: the backward pass must agree
    int fwd_gemm_arith = 0;   // ... and the general matrix route in this arithmetic: the reverse pass recomputes expConv and must get the forward's gates
    bool fwd_gemm_exotic = false;   // ... and the exotic launches on this side of the fourth switch: the slab regions of the reverse scratch follow it
    // optional per-kernel-class timing with HIP events on the launch stream (bench.py's roofline leg)
    bool prof_on = false;
    unsigned prof_mask = ~0u;   // kernel classes whose launches are bracketed (bit = class index)
    std::vector<hipEvent_t> prof_ev;
    std::vector<int> prof_cls;
    std::vector<double> prof_macs;
    size_t prof_used = 0;
};

// the family of the engine's impl and its four switches: every setter makes it here, so each keeps what the others set
static Family engine_family(const probav_engine* e) { return make_family(e->impl, e->pw_mfma, e->gemm, e->gemm_pair && e->pw_gemm, e->gemm_x6, e->gemm_exotic); }

enum { CLS_WN = 0, CLS_SMALL, CLS_CONV3_FWD, CLS_CONV3_BWD_DATA, CLS_CONV3_WGRAD, CLS_PW_FWD, CLS_PW_BWD_DATA, CLS_PW_WGRAD,
       // launches served by an x6 kernel (bf16 MFMA pipe) are timed apart from the fp32-MFMA / VALU ones: they price against another peak
       CLS_CONV3_FWD_X6, CLS_CONV3_BWD_DATA_X6, CLS_CONV3_WGRAD_X6, CLS_PW_FWD_X6, CLS_PW_BWD_DATA_X6, CLS_COUNT };

struct ProfScope {
    probav_engine* e; hipStream_t s; bool live;
    ProfScope(const probav_engine* ce, int cls, double macs, hipStream_t st) : e(const_cast<probav_engine*>(ce)), s(st), live(false)
    {
        if (!e->prof_on || !((e->prof_mask >> cls) & 1u) || e->prof_used + 2 > e->prof_ev.size()) return;
        if (e->side.side && st == e->side.side) return;    // launches on the side stream run in the gaps of the caller's chain: events around them would time the chain, not them
        live = true;
        e->prof_cls.push_back(cls);
        e->prof_macs.push_back(macs);
        (void)hipEventRecord(e->prof_ev[e->prof_used], s);
    }
    ~ProfScope()
    {
        if (!live) return;
        (void)hipEventRecord(e->prof_ev[e->prof_used + 1], s);
        e->prof_used += 2;
    }
};
static double geom_macs(const ConvGeom& g)
{
    return (double)g.N * g.Ho * g.Wo * g.To * g.kh * g.kw * g.kt * g.Cin * g.Cout;
}

static int add_layer(probav_engine* e, const std::string& name, int kh, int kw, int kt, int cin, int cout)
{
    LayerRec r = {};
    snprintf(r.name, sizeof(r.name), "%s", name.c_str());
    r.kh = kh; r.kw = kw; r.kt = kt;
    r.wn.taps = kh * kw * kt; r.wn.Cin = cin; r.wn.Cout = cout; r.wn.K = r.wn.taps * cin;
    r.wn.g_off = (int)e->nparams;
    r.wn.v_off = r.wn.g_off + cout;
    r.wn.b_off = r.wn.v_off + r.wn.K * cout;
    r.wn.w_off = (int)e->weff_count;
    r.wn.n_off = (int)e->cout_total;
    r.wn.r_off = (int)e->cin_total;
    e->nparams += 2 * cout + (int64_t)r.wn.K * cout;
    e->weff_count += (int64_t)r.wn.K * cout;
    e->cout_total += cout;
    e->cin_total += cin;
    e->layers.push_back(r);
    return (int)e->layers.size() - 1;
}

static size_t align_up(size_t v) { return (v + 63) & ~(size_t)63; }      // 64 floats = 256 B

// The network's geometry for one (engine, batch): the forward ConvGeom of every layer (a reducer's input extents are its Hi, Ti).  make_net is
// the one place that states them; the plan, both passes and the introspection calls read them here (backward-data: bwd_data_geom of these)
struct Net {
    ConvGeom main, exp, dec, norm, up, resid1, resid2, resid3;      // exp / dec / norm: the same for every block
    std::vector<ConvGeom> red;
};
static size_t in_floats(const ConvGeom& g) { return (size_t)g.N * g.Hi * g.Wi * g.Ti * g.Cin; }
static size_t out_floats(const ConvGeom& g) { return (size_t)g.N * g.Ho * g.Wo * g.To * g.Cout; }
static long in_voxels(const ConvGeom& g) { return (long)g.N * g.Hi * g.Wi * g.Ti; }

// Which operands a launch has: all that the route functions (conv_route, wgrad_route) need to know of them
struct Operands {
    bool gate = false, bias = false, skip = false;
    bool f32 = false, x6 = false, h3 = false, h3t = false;    // the filter fragments that exist (h3t: per-tap H3 fragments of a 25-channel layer)
    bool am_in = false;                                       // the launch gets the amax slots of its inputs (Amax: x and w)
    bool am_out = false;                                      // ... and must leave its output's amax (Amax: y)
};

// One routed launch of a training step.  step_launches lists them, forward then backward, in issue order: the one statement of which launches a step consists
// of.  make_plan lays the slab regions out and counts the amax slots over it, probav_engine_route_counts routes it, and the passes fetch every launch here by its site
enum class Role { resid1, resid2, resid3, resid_path, main, exp, dec, pair, norm, red, up, hidden };   // pair / resid_path: the fused launches; hidden: expConv's output recomputed by the un-fused reverse pass
enum class LaunchKind { none, conv, wgrad, fused };          // conv: forward, or in the reverse pass backward-data (hidden: forward); wgrad: backward-filter; fused: the pointwise pair or the residual path, one launch each way
struct Region { static constexpr size_t none = ~(size_t)0; size_t off = none, floats = 0; };     // of the scratch's slab area: offset relative to Plan::partial, size
struct Launch {
    Role role = Role::main; int i = 0;                        // the site: whose launch (i: block or reducer) ...
    LaunchKind kind = LaunchKind::none; bool back = false;    // ... and which of them, of which pass
    ConvGeom g;                                               // the geometry launched (backward-data: bwd_data_geom of the layer's; fused: of the pair's / the path's first layer)
    int li = -1, dir = -1;                                    // the layer and the direction of its fragments (0 forward, 1 backward-data, -1: the launch has none)
    Operands o;                                               // as the pass hands them over
    int slots = 0, slot = -1;                                 // reverse pass: per-sample amax slot arrays its output takes (2: one more for the fold of its mirrored pads), the first's index
    Region slab;                                              // backward-filter and fused reverse launches: the slab region
};

struct Plan {
    Net net;
    std::vector<Launch> launches;
    size_t weff, weffT, invn, xn, mn;
    size_t amax; int n_amax, amax_bwd, amax_fwd, B;   // amax slots (one 32-bit word each, x6_device.h): region offset, count, first slot of the backward / forward per-sample arrays
    int n_back;                               // per-sample slot arrays the reverse pass takes (Launch::slots); the region behind amax_bwd holds at least as many
    std::vector<size_t> act, dec, red;
    size_t up, r1, r2, r3, H, wpack;
    // --- what only the reverse pass writes (offsets relative to the SCRATCH base: the tail of a one-piece workspace, or the caller's second buffer) ---
    size_t bamax, dweff2, Hb, dH, gA, gB, gDec, dtail, dr2, dr1, partial;
    size_t fwd_total, bwd_total, total;       // floats: the saved state of a forward pass | the reverse pass's scratch | both
    std::vector<size_t> gblk, gred;
};
// the launch at a site, or an entry of kind none (which conv_fwd / conv_wgrad refuse): by value, so that a queued launch may keep it
static Launch launch_at(const Plan& p, Role role, LaunchKind kind, bool back, int i = 0)
{
    for (const Launch& L : p.launches) if (L.role == role && L.kind == kind && L.back == back && L.i == i) return L;
    Launch none; none.role = role; none.back = back; none.i = i;
    return none;
}

static ConvGeom make_geom(int N, int Hi, int Ti, int Cin, int Ho, int To, int Cout, int kh, int kw, int kt,
                          int ph, int pt, int reflect, int relu)
{
    ConvGeom g;
    g.N = N; g.Hi = Hi; g.Wi = Hi; g.Ti = Ti; g.Cin = Cin; g.Ho = Ho; g.Wo = Ho; g.To = To; g.Cout = Cout;
    g.kh = kh; g.kw = kw; g.kt = kt; g.ph = ph; g.pw = ph; g.pt = pt; g.reflect_hw = reflect; g.relu = relu; g.reflect_t = 0;
    return g;
}

// backward-data geometry of a forward layer: a correlation of dy with the flipped, channel-swapped
// kernel and padding k-1-p; for reflect layers the result is the gradient of the PADDED input.
static ConvGeom bwd_data_geom(const ConvGeom& f)
{
    ConvGeom b = f;
    const int php = f.reflect_hw ? 0 : f.ph, pwp = f.reflect_hw ? 0 : f.pw, ptp = f.reflect_t ? 0 : f.pt;
    b.Hi = f.Ho; b.Wi = f.Wo; b.Ti = f.To; b.Cin = f.Cout;
    b.Ho = f.reflect_hw ? f.Hi + 2 * f.ph : f.Hi;
    b.Wo = f.reflect_hw ? f.Wi + 2 * f.pw : f.Wi;
    b.To = f.reflect_t ? f.Ti + 2 * f.pt : f.Ti;
    b.Cout = f.Cin;
    b.ph = f.kh - 1 - php; b.pw = f.kw - 1 - pwp; b.pt = f.kt - 1 - ptp;
    b.reflect_hw = 0; b.reflect_t = 0; b.relu = 0;
    return b;
}

// geometry of reducer k on an input of extent h x h x t
static ConvGeom red_geom(const probav_engine* e, int B, size_t k, int h, int t, int F)
{
    const probav_engine::RedSpec& r = e->redSpec[k];
    ConvGeom g = make_geom(B, h, t, F, h + 2 * r.p - (r.k - 1), t + 2 * r.pt - (r.k - 1), F, r.k, r.k, r.k, r.p, r.pt, r.refl, 1);
    g.reflect_t = r.refl_t;
    return g;
}

static Net make_net(const probav_engine* e, int B)
{
    const probav_net_cfg& c = e->cfg;
    const int F = c.num_filters, E = F * c.exp_rate, D = c.dec_channels, T = c.num_img_lr, Cx = c.in_channels;
    const int Hin = e->Hin, P = c.patch_size_lr, s2 = c.scale * c.scale;
    Net n;
    //                  N  Hi       Ti Cin Ho       To Cout kh kw kt ph pt reflect relu
    n.main   = make_geom(B, Hin,     T, Cx, Hin,     T, F,   3, 3, 3, 1, 1, 0, 1);
    n.exp    = make_geom(B, Hin,     T, F,  Hin,     T, E,   1, 1, 1, 0, 0, 0, 1);
    n.dec    = make_geom(B, Hin,     T, E,  Hin,     T, D,   1, 1, 1, 0, 0, 0, 0);
    n.norm   = make_geom(B, Hin,     T, D,  Hin,     T, F,   3, 3, 3, 1, 1, 0, 0);
    int h = Hin, t = T;
    for (size_t k = 0; k < e->redSpec.size(); ++k) {
        n.red.push_back(red_geom(e, B, k, h, t, F));
        h = n.red[k].Ho; t = n.red[k].To;
    }
    n.up     = make_geom(B, h,       t, F,  P,       1, s2,  3, 3, 3, 0, 0, 0, 0);
    n.resid1 = make_geom(B, Hin,     1, Cx, Hin - 2, 1, s2,  3, 3, 1, 0, 0, 0, 1);
    n.resid2 = make_geom(B, Hin - 2, 1, s2, Hin - 4, 1, s2,  3, 3, 1, 0, 0, 0, 0);
    n.resid3 = make_geom(B, Hin - 4, 1, s2, P,       1, s2,  3, 3, 1, 0, 0, 0, 0);
    return n;
}

// the low-frequency residual path runs as one launch each way (kernels_direct.hip: resid_path_*) in every family but 0, which stays on the generic direct kernels
static bool resid_path_fused(const probav_engine* e)
{
    return e->fam.mfma && resid_path_supported(e->Hin, e->cfg.in_channels, e->cfg.scale * e->cfg.scale);
}

// The kernel that serves a backward-filter launch: the one decision both make_plan (slab region sizes) and conv_wgrad (launch) read.
// o.am_in: the launch has the per-sample amax slots of x and of dy (the H3 kernel needs both).  tuned: the direct kernel's dedicated small instance
enum class WgradKernel { direct, x6, mfma, gemm };
struct WgradRoute { WgradKernel k; int cls; int arith; bool tuned; bool wide = false; };     // wide: the route's kernel through its wide predicate (an exotic geometry)
static WgradRoute wgrad_route(const Family& f, const ConvGeom& g, const Operands& o)
{
    const bool exotic = g.reflect_t || g.ph > 1 || g.pw > 1 || g.pt > 1 || (g.kh != 3 && g.kh != 1);
    const bool tuned = f.mfma && conv3d_direct_wgrad_is_tuned(g);
    // the fourth switch: an exotic geometry on the route's kernel where the wide predicate takes it (fp32, as the route's other backward-filters)
    if (exotic && !tuned && f.gemm_exotic && gemm_wgrad_supported_wide(g)) return {WgradKernel::gemm, CLS_CONV3_WGRAD, 0, false, true};
    if (exotic || tuned) return {WgradKernel::direct, CLS_CONV3_WGRAD, 0, tuned};
    const bool x6 = f.x6 && x6_wgrad_supported(g);
    const int cls = g.kh * g.kw * g.kt == 1 ? CLS_PW_WGRAD : (x6 ? CLS_CONV3_WGRAD_X6 : CLS_CONV3_WGRAD);
    if (x6) return {WgradKernel::x6, cls, f.arith == 2 && o.am_in ? 2 : 1, false};
    if (f.mfma && mfma_wgrad_supported(g)) return {WgradKernel::mfma, cls, 0, false};
    // the general matrix route: only what would be the generic direct kernel's.  fp32 whatever the route's third switch says (Family::gemm_arith covers its
    // convolution launches only: an x6 backward-filter was measured slower than this kernel)
    if (f.gemm && gemm_wgrad_supported(g)) return {WgradKernel::gemm, cls, 0, false};
    return {WgradKernel::direct, cls, 0, false};
}
// the slot of the launch census (probav_engine_route_counts, probav_engine_launched_counts) a routed backward-filter counts in, or -1
static int census_slot(const WgradRoute& r) { return r.k == WgradKernel::gemm ? 3 : (r.k == WgradKernel::direct && !r.tuned ? 2 : -1); }
// slab floats the routed kernel writes
static size_t wgrad_slab_floats(const WgradRoute& r, const ConvGeom& g)
{
    if (r.k == WgradKernel::gemm) return gemm_wgrad_partial_floats(g);
    return r.k == WgradKernel::x6 ? x6_wgrad_partial_floats(g) : (r.k == WgradKernel::mfma ? mfma_wgrad_partial_floats(g) : wgrad_partial_floats(g));
}
static size_t wgrad_need(const Family& f, const ConvGeom& g, const Operands& o = Operands()) { return wgrad_slab_floats(wgrad_route(f, g, o), g); }

// The launches of one training step on the network n.  The family-dependent shape of the step is stated here and nowhere else: the residual path and the
// pointwise pair fused or layer by layer, and under the H3 arithmetic which launches get their inputs' amax slots and which leave their output's
static std::vector<Launch> step_launches(const probav_engine* e, const Net& n)
{
    const bool h3 = e->fam.arith == 2, fusedp = e->fam.pw_fused != PairKind::none, fusedr = resid_path_fused(e);
    const int R = e->cfg.num_res_blocks, nred = (int)n.red.size();
    std::vector<Launch> v;
    v.reserve(16 + 12 * R + 4 * nred);
    auto add = [&](Role role, int i, LaunchKind kind, bool back, const ConvGeom& g, int li, int dir) -> Launch& {
        Launch L; L.role = role; L.i = i; L.kind = kind; L.back = back; L.g = g; L.li = li; L.dir = dir;
        v.push_back(L);
        return v.back();
    };
    // dir 0: the layer's forward; 1: its backward-data; -1: its forward again, without fragments.  in / out: the amax slots under H3
    auto conv = [&](Role role, int i, const ConvGeom& g, int li, int dir, bool gate, bool skip, bool in, bool out, int slots = 0) {
        Launch& L = add(role, i, LaunchKind::conv, dir != 0, dir == 1 ? bwd_data_geom(g) : g, li, dir);
        if (dir >= 0) { const ConvFrags& c = e->layers[li].pk[dir]; L.o.f32 = c.f32 >= 0; L.o.x6 = c.x6 >= 0; L.o.h3 = c.h3 >= 0; L.o.h3t = c.h3t >= 0; }
        L.o.gate = gate; L.o.bias = dir != 1; L.o.skip = skip; L.o.am_in = h3 && in; L.o.am_out = h3 && out; L.slots = slots;
    };
    auto wgrad = [&](Role role, int i, const ConvGeom& g, int li, bool gate, bool in) {
        Launch& L = add(role, i, LaunchKind::wgrad, true, g, li, -1);
        L.o.gate = gate; L.o.am_in = h3 && in;
    };
    // forward (forward_impl)
    if (fusedr) add(Role::resid_path, 0, LaunchKind::fused, false, n.resid1, -1, -1);
    else {
        conv(Role::resid1, 0, n.resid1, e->iResid1, 0, false, false, false, false);
        conv(Role::resid2, 0, n.resid2, e->iResid2, 0, false, false, false, false);
        conv(Role::resid3, 0, n.resid3, e->iResid3, 0, false, false, false, false);
    }
    conv(Role::main, 0, n.main, e->iMain, 0, false, false, false, true);
    for (int i = 0; i < R; ++i) {
        if (fusedp) add(Role::pair, i, LaunchKind::fused, false, n.exp, -1, -1);
        else {
            conv(Role::exp, i, n.exp, e->iExp[i], 0, false, false, false, false);
            conv(Role::dec, i, n.dec, e->iDec[i], 0, false, false, false, true);
        }
        conv(Role::norm, i, n.norm, e->iNorm[i], 0, false, true, true, true);
    }
    for (int k = 0; k < nred; ++k) conv(Role::red, k, n.red[k], e->iRed[k], 0, false, false, true, true);
    conv(Role::up, 0, n.up, e->iUp, 0, false, false, true, false);
    // backward (backward_impl): the residual path last layer first, upscale layer, reducers, blocks, mainConv1 (input-facing: no backward-data)
    if (fusedr) add(Role::resid_path, 0, LaunchKind::fused, true, n.resid1, -1, -1);
    else {
        wgrad(Role::resid3, 0, n.resid3, e->iResid3, false, false);
        conv(Role::resid3, 0, n.resid3, e->iResid3, 1, false, false, false, false);
        wgrad(Role::resid2, 0, n.resid2, e->iResid2, false, false);
        conv(Role::resid2, 0, n.resid2, e->iResid2, 1, false, false, false, false);
        wgrad(Role::resid1, 0, n.resid1, e->iResid1, true, false);
    }
    wgrad(Role::up, 0, n.up, e->iUp, false, false);
    conv(Role::up, 0, n.up, e->iUp, 1, false, false, false, true, 1);
    for (int k = nred - 1; k >= 0; --k) {
        wgrad(Role::red, k, n.red[k], e->iRed[k], true, true);
        conv(Role::red, k, n.red[k], e->iRed[k], 1, true, false, true, true, n.red[k].reflect_hw ? 2 : 1);     // (the folded gradient of mirrored pads is a new tensor)
    }
    for (int i = R - 1; i >= 0; --i) {
        wgrad(Role::norm, i, n.norm, e->iNorm[i], false, true);
        conv(Role::norm, i, n.norm, e->iNorm[i], 1, false, false, true, true, 1);
        if (fusedp) { add(Role::pair, i, LaunchKind::fused, true, n.exp, -1, -1).slots = 1; continue; }
        conv(Role::hidden, i, n.exp, e->iExp[i], -1, false, false, false, false);
        wgrad(Role::dec, i, n.dec, e->iDec[i], false, false);
        conv(Role::dec, i, n.dec, e->iDec[i], 1, false, false, false, false);
        wgrad(Role::exp, i, n.exp, e->iExp[i], true, false);
        conv(Role::exp, i, n.exp, e->iExp[i], 1, true, true, false, true, 1);
    }
    wgrad(Role::main, 0, n.main, e->iMain, true, false);
    return v;
}

// slab floats of the fused pair's reverse launch (g: expConv's geometry), by the kind that runs it
static size_t pair_slab_floats(const probav_engine* e, const ConvGeom& g)
{
    if (e->fam.pw_fused == PairKind::gemm) return gemm_pw_backward_slab_floats(g.Cin, g.Cout, e->cfg.dec_channels, in_voxels(g));
    return mfma_pw_backward_slab_floats(e->cfg.dec_channels);
}

static Plan make_plan(const probav_engine* e, int B, int training)
{
    Plan p;
    p.net = make_net(e, B);
    p.launches = step_launches(e, p.net);
    const Net& n = p.net;
    const int R = e->cfg.num_res_blocks, nred = (int)n.red.size();
    size_t off = 0;
    auto take = [&](size_t q) { size_t o = off; off += align_up(q); return o; };
    p.weff = take(e->weff_count); p.weffT = take(e->weff_count); p.invn = take(e->cout_total);
    {   // slots: per layer [weights | biases] (whole tensor), per output channel, per input channel (wn_forward's layout); then ONE SLOT PER
        // SAMPLE for act[0..R], dec[0..R-1], the reducer outputs, and for the backward pass's tensors in launch order: the upscale layer's input
        // gradient, per reducer its input gradient and (mirrored pads) the folded one, per block those of dec_i and act[i]
        const int L = (int)e->layers.size();
        p.B = B;
        p.amax_fwd = 2 * L + (int)e->cout_total + (int)e->cin_total;
        p.amax_bwd = p.amax_fwd + B * (2 * R + 1 + nred);
        p.n_back = 0;
        for (Launch& L : p.launches) if (L.slots) { L.slot = p.n_back; p.n_back += L.slots; }
        p.n_amax = p.amax_bwd + (training ? B * (2 * R + 2 * nred + 8) : 0);     // (reserved: n_back and a margin that the workspace sizes have always carried)
        p.amax = take((size_t)p.amax_bwd);
    }
    p.wpack = take(e->wpack_count);
    p.xn = take(in_floats(n.main)); p.mn = take(in_floats(n.resid1));
    if (training) {
        for (int i = 0; i <= R; ++i) p.act.push_back(take(out_floats(n.main)));
        for (int i = 0; i < R; ++i) p.dec.push_back(take(out_floats(n.dec)));
    } else {
        const size_t a0 = take(out_floats(n.main)), a1 = take(out_floats(n.main)), d0 = take(out_floats(n.dec));
        for (int i = 0; i <= R; ++i) p.act.push_back((i & 1) ? a1 : a0);
        for (int i = 0; i < R; ++i) p.dec.push_back(d0);
    }
    for (const ConvGeom& g : n.red) p.red.push_back(take(out_floats(g)));
    p.up = take(out_floats(n.up));
    p.r1 = take(out_floats(n.resid1));
    p.r2 = take(out_floats(n.resid2));
    p.r3 = take(out_floats(n.resid3));
    // the 256-channel hidden tensor (1 KB per voxel) only exists in memory when the pointwise pair runs UNfused (generic kernels, impl 0)
    const bool unfused = e->fam.pw_fused == PairKind::none;
    p.H = take(unfused ? out_floats(n.exp) : 0);
    p.fwd_total = off;
    off = 0;
    p.bamax = p.dweff2 = p.Hb = p.dH = p.gA = p.gB = p.gDec = p.dtail = p.dr2 = p.dr1 = p.partial = 0;
    if (training) {
        p.bamax = take((size_t)(p.n_amax - p.amax_bwd));
        p.dweff2 = take(e->weff_count);
        p.Hb = take(unfused ? out_floats(n.exp) : 0);  // the recomputed hidden tensor of the unfused path (the forward pass's own copy is saved state: read-only here)
        // gradient buffers of the chain: the largest (mirror-padded) reducer input, and never less than a block-sized tensor padded by one row / column
        size_t gmax = (size_t)B * (n.main.Ho + 2) * (n.main.Wo + 2) * n.main.To * n.main.Cout;
        for (const ConvGeom& g : n.red) gmax = std::max(gmax, out_floats(bwd_data_geom(g)));
        p.gA = take(gmax); p.gB = take(gmax); p.gDec = take(out_floats(n.dec));
        // every block's input gradient in its own buffer: the block's backward-filter (needed only by the weight-norm backward at the very end)
        // runs on the low-priority side stream, filling the tails of the main chain's launches, and must find its dY untouched whenever it runs
        for (int i = 0; i < R; ++i) p.gblk.push_back(take(out_floats(n.main)));
        for (int k = 0; k < 2 * nred; ++k) p.gred.push_back(take(gmax));   // the reducers likewise: backward-data output and (mirrored pads) its folded form
        p.dtail = take(out_floats(n.up));
        p.dr2 = take(out_floats(n.resid2));
        p.dr1 = take(out_floats(n.resid1));
        p.dH = take(unfused ? out_floats(n.exp) : 0);
        // one slab region per launch of the reverse pass that writes slabs, in list order: the slabs of a launch are summed on the side stream while the
        // main chain has moved on, so no two launches may share a region
        size_t acc = 0;
        auto region = [&](size_t q) { Region r; r.off = acc; r.floats = q; acc += align_up(q); return r; };
        for (Launch& L : p.launches) {
            if (!L.back) continue;
            if (L.kind == LaunchKind::wgrad) L.slab = region(wgrad_need(e->fam, L.g, L.o));
            else if (L.kind == LaunchKind::fused && L.role == Role::pair) L.slab = region(pair_slab_floats(e, L.g));
            else if (L.kind == LaunchKind::fused) {
                // the fused residual path: one slab per patch in the first of the three regions its layers would have, which keep the sizes they have always had,
                // with or without the general matrix route
                Family fr = e->fam; fr.gemm = false;
                L.slab = region(std::max(wgrad_need(fr, n.resid3), resid_path_slab_floats(B, n.resid1.Cin)));
                region(wgrad_need(fr, n.resid2)); region(wgrad_need(fr, n.resid1));
            }
        }
        p.partial = take(acc);
    }
    p.bwd_total = off;
    p.total = p.fwd_total + p.bwd_total;
    return p;
}

// Weight cache (optional, caller-owned): everything a forward / backward pass derives from the parameters alone -- effective weights in
// both layouts, inverse norms, the weights' amax slots, the packed MFMA operand fragments.  probav_optimizer_step_fused fills it for the
// parameters it has just updated; the *_wc entry points then skip the weight-norm and packing launches.
struct WcPlan { size_t weff, weffT, invn, amax, wpack, total; int n_wamax; };
static WcPlan make_wc_plan(const probav_engine* e)
{
    WcPlan c; size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += align_up(n); return o; };
    c.weff = take(e->weff_count); c.weffT = take(e->weff_count); c.invn = take(e->cout_total);
    c.n_wamax = 2 * (int)e->layers.size() + (int)e->cout_total + (int)e->cin_total;
    c.amax = take((size_t)c.n_wamax); c.wpack = take(e->wpack_count);
    c.total = off;
    return c;
}

// ---------------------------------------------------------------------------------------------------
// Where the parameter-derived tensors of a pass live: in the caller's weight cache (WC), or in the workspace W, where the forward pass recomputes them.
// wslots: the weights' amax slots (the head of the workspace's amax region, or the cache's)
struct Derived { const float *weff, *weffT, *invn, *wpack; unsigned* wslots; };
static Derived derived(const probav_engine* e, const Plan& p, const float* W, const float* WC)
{
    auto slots = [](const float* q) { return reinterpret_cast<unsigned*>(const_cast<float*>(q)); };
    if (!WC) return {W + p.weff, W + p.weffT, W + p.invn, W + p.wpack, slots(W + p.amax)};
    const WcPlan wc = make_wc_plan(e);
    return {WC + wc.weff, WC + wc.weffT, WC + wc.invn, WC + wc.wpack, slots(WC + wc.amax)};
}

// amax slot addresses inside the workspace (layout: make_plan)
struct AmaxSlots {
    const probav_engine* e; unsigned* base; unsigned* wbase; unsigned* bbase; int L, R, B, fwd;
    // wslots: where the weights' slots live (Derived); S: the reverse pass's scratch (its slots live there)
    AmaxSlots(const probav_engine* e_, const Plan& p, const float* W, unsigned* wslots, float* S = nullptr)
        : e(e_), base(reinterpret_cast<unsigned*>(const_cast<float*>(W) + p.amax)), wbase(wslots),
          bbase(S ? reinterpret_cast<unsigned*>(S + p.bamax) : nullptr), L((int)e_->layers.size()), R(e_->cfg.num_res_blocks), B(p.B), fwd(p.amax_fwd) {}
    unsigned* w(int li) const { return wbase + li; }                                   // whole weight tensor of layer li
    unsigned* b(int li) const { return wbase + L + li; }                               // its bias
    unsigned* wcol(int li) const { return wbase + 2 * L + e->layers[li].wn.n_off; }     // per output channel (Cout slots): columns of the forward matrices
    unsigned* wrow(int li) const { return wbase + 2 * L + (int)e->cout_total + e->layers[li].wn.r_off; }   // per input channel (Cin slots): columns of the backward-data matrices
    unsigned* act(int i) const { return base + fwd + B * i; }                         // per-sample arrays (B slots each)
    unsigned* dec(int i) const { return base + fwd + B * (R + 1 + i); }
    unsigned* red(int k) const { return base + fwd + B * (2 * R + 1 + k); }
    unsigned* back(int j) const { return bbase + B * j; }                             // j-th tensor produced by the backward pass
};

// The kernel that serves a convolution launch of the engine (forward, or backward-data when it has no bias): with the launch's profiling class,
// whether the kernel writes am.y itself, and for the MFMA / x6 kernels the kind of filter fragments they read (x6: in arithmetic 1 X6 or 2 H3)
enum class ConvKernel { direct, up, up_bwd_data, cin1, x6_strip, x6_rowtile, mfma_strip, mfma_rowtile, gemm };
enum class FragKind { none, f32, x6, h3, h3t };
struct ConvRoute { ConvKernel k; int cls; bool reports; int arith; FragKind frag; StripSel strip; bool wide = false; };     // strip: the strip kernels' selection (strip_select), made here once
// `dedicated`: the engine's policy in front of the matrix kernels (small dedicated kernels, exotic geometries on the direct one); the single-operator entry point,
// whose tests hold the matrix kernels to the oracle on those geometries too, routes without it
static ConvRoute conv_route(const Family& f, const ConvGeom& g, const Operands& o, bool dedicated = true)
{
    const bool pw = g.kh * g.kw * g.kt == 1;
    const bool bwd = !o.bias;                        // only backward-data launches run without a bias
    if (dedicated) {
        // the experimental 19-frame reducer: 5x5x5 kernels, pads of 2, mirrored depth pads (and their backward-data forms): generic kernels
        const bool exotic = g.reflect_t || g.ph > 2 || g.pw > 2 || g.pt > 2 || (!pw && g.kh != 3) || (g.reflect_hw && g.ph > 1);
        // upscaleConv1 and its backward-data (0.2 % of the work): dedicated small VALU kernels instead of 32x32 matrix tiles around a 32x9 product
        if (f.mfma && !o.gate && !o.skip && bwd && conv3d_up_bwd_data_supported(g)) return {ConvKernel::up_bwd_data, CLS_CONV3_BWD_DATA, true, 0, FragKind::none, {}};
        // the fourth switch: an exotic geometry on the route's kernels where the wide predicate takes it, in the route's arithmetic
        if (exotic && f.gemm_exotic && gemm_conv_supported_wide(g))
            return {ConvKernel::gemm, f.gemm_arith ? (bwd ? CLS_CONV3_BWD_DATA_X6 : CLS_CONV3_FWD_X6) : (bwd ? CLS_CONV3_BWD_DATA : CLS_CONV3_FWD), false, f.gemm_arith, FragKind::none, {}, true};
        if (exotic) return {ConvKernel::direct, bwd ? CLS_CONV3_BWD_DATA : CLS_CONV3_FWD, false, 0, FragKind::none, {}};
        if (f.mfma && !o.gate && !o.skip && o.bias && !o.am_out && conv3d_up_forward_supported(g)) return {ConvKernel::up, CLS_CONV3_FWD, false, 0, FragKind::none, {}};
        if (f.mfma && !o.gate && !o.skip && o.bias && conv3d_cin1_forward_supported(g)) return {ConvKernel::cin1, CLS_CONV3_FWD, true, 0, FragKind::none, {}};
    }
    const bool h3 = f.arith == 2 && o.h3 && o.am_in;
    const FragKind wsplit = h3 ? FragKind::h3 : FragKind::x6;
    const int arith = h3 ? 2 : 1;
    const bool split = f.x6 && (h3 || o.x6);
    const StripSel sel = split ? strip_select(g, o.gate, arith) : StripSel();
    const bool x6s = sel.k != StripKernel::none;
    const bool x6r = split && !x6s && x6_conv_rowtile_supported(g);
    const bool x6 = x6s || x6r;
    const int cls = pw ? (bwd ? CLS_PW_BWD_DATA : CLS_PW_FWD) : (bwd ? (x6 ? CLS_CONV3_BWD_DATA_X6 : CLS_CONV3_BWD_DATA) : (x6 ? CLS_CONV3_FWD_X6 : CLS_CONV3_FWD));
    if (x6s) return {ConvKernel::x6_strip, cls, true, arith, (sel.taps && g.Cin == 25 && o.h3t) ? FragKind::h3t : wsplit, sel};
    if (x6r) return {ConvKernel::x6_rowtile, cls, true, arith, wsplit, {}};
    const StripSel s32 = (f.strip && o.f32 && !split) ? strip_select(g, o.gate, 0) : StripSel();      // (split: no strip kernel took g above, so the fp32 one does not either)
    if (s32.k != StripKernel::none) return {ConvKernel::mfma_strip, cls, true, 0, FragKind::f32, s32};
    if (f.mfma && o.f32 && mfma_conv_supported(g)) return {ConvKernel::mfma_rowtile, cls, true, 0, FragKind::f32, {}};
    // the general matrix route: what no matrix, split-operand or dedicated kernel took above (an exotic geometry returned before).  It does not report amax
    // In x6 arithmetic (arith 1, the _X6 profiling classes) where the third switch is on
    if (f.gemm && dedicated && gemm_conv_supported(g)) {
        const int xcls = pw ? (bwd ? CLS_PW_BWD_DATA_X6 : CLS_PW_FWD_X6) : (bwd ? CLS_CONV3_BWD_DATA_X6 : CLS_CONV3_FWD_X6);
        return {ConvKernel::gemm, f.gemm_arith ? xcls : cls, false, f.gemm_arith, FragKind::none, {}};
    }
    return {ConvKernel::direct, cls, false, 0, FragKind::none, {}};
}
static int census_slot(const ConvRoute& r) { return r.k == ConvKernel::direct ? 0 : (r.k == ConvKernel::gemm ? 1 : -1); }      // (as census_slot of a backward-filter route)
// the routed launch (w: the filter as the direct kernels read it; wfrag: its fragments of the kind the route chose)
static int conv_launch(const ConvRoute& r, const ConvGeom& g, const float* x, const float* gate, const float* w, const float* wfrag, const float* bias,
                       const float* skip, float* y, const Amax& am, hipStream_t s)
{
    switch (r.k) {
    case ConvKernel::up_bwd_data: return conv3d_up_bwd_data(g, x, w, nullptr, y, am.y, s);
    case ConvKernel::up: return conv3d_up_forward(g, x, w, bias, y, s);
    case ConvKernel::cin1: return conv3d_cin1_forward(g, x, w, bias, y, am.y, s);
    case ConvKernel::x6_strip: case ConvKernel::mfma_strip: return conv_strip_forward(r.strip, x, gate, wfrag, bias, skip, y, am, s);
    case ConvKernel::x6_rowtile: return x6_conv_rowtile_forward(g, x, gate, wfrag, bias, skip, y, r.arith, am, s);
    case ConvKernel::mfma_rowtile: return mfma_conv_forward(g, x, gate, wfrag, bias, skip, y, am, s);
    case ConvKernel::gemm:
        if (r.wide) return r.arith ? gemm_x6_conv_forward_wide(g, x, gate, w, bias, skip, y, s) : gemm_conv_forward_wide(g, x, gate, w, bias, skip, y, s);
        return r.arith ? gemm_x6_conv_forward(g, x, gate, w, bias, skip, y, s) : gemm_conv_forward(g, x, gate, w, bias, skip, y, s);
    default: return conv3d_direct_forward(g, x, gate, w, bias, skip, y, s);
    }
}

#define CK(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)

// What a pass hands over with a launch must be what its entry of the launch list states: the plan and the census have routed and sized the launch by the entry
// (weights, bias and fragments are the entry's own: conv_fwd / conv_wgrad take them from its layer).  A host comparison, made before anything is launched
static int operands_agree(const Launch& L, LaunchKind kind, const float* gate, const float* skip, const Amax& am)
{
    const Operands& o = L.o;
    if (L.kind == kind && (gate != nullptr) == o.gate && (skip != nullptr) == o.skip && (am.x && am.w) == o.am_in && (am.y != nullptr) == o.am_out) return PROBAV_OK;
    static const char* const roles[] = {"residConv1", "residConv2", "residConv3", "the residual path", "mainConv1", "expConv", "decConv", "the pointwise pair", "normConv", "convReducer", "upscaleConv1", "expConv (recomputed)"};
    set_error((std::string("probav engine: the ") + (L.back ? "reverse" : "forward") + " pass's " + (kind == LaunchKind::wgrad ? "backward-filter" : "convolution") + " launch of " + roles[(int)L.role] +
               " [" + std::to_string(L.i) + "] " + (L.kind == LaunchKind::none ? "is not in the launch list" : "has other operands than the launch list states")).c_str(), hipSuccess);
    return PROBAV_EINVAL;
}
// Where a pass's launches find what the layer tables determine: the parameter-derived tensors and, reverse pass, the gradient and slab areas.  Copied into queued launches
struct PassBufs { const probav_engine* e; Derived dv; const float* params; float *dweff2, *grads, *slabs; };
// am.x / am.w: amax slots of x (one per sample) and of the layer's filter columns (H3 kernels); am.y: per-sample slots that must hold the output's amax afterwards
static int conv_fwd(const PassBufs& b, const Launch& L, const float* x, const float* gate, const float* skip, float* y, const Amax& am, hipStream_t s)
{
    const probav_engine* e = b.e;
    const ConvGeom& g = L.g;
    CK(operands_agree(L, LaunchKind::conv, gate, skip, am));
    const WnLayer& wn = e->layers[L.li].wn;
    const float* w = (L.dir == 1 ? b.dv.weffT : b.dv.weff) + wn.w_off;
    const float* bias = L.o.bias ? b.params + wn.b_off : nullptr;
    const ConvRoute r = conv_route(e->fam, g, L.o);
    if (census_slot(r) >= 0) ++const_cast<probav_engine*>(e)->launched[census_slot(r)];
    // the fragments of the kind the route chose, in the packed region (a route only chooses a kind that L.o states, so the layer has it in direction L.dir)
    const ConvFrags nofrags, &c = L.dir < 0 ? nofrags : e->layers[L.li].pk[L.dir];
    const long foff = r.frag == FragKind::f32 ? c.f32 : (r.frag == FragKind::x6 ? c.x6 : (r.frag == FragKind::h3 ? c.h3 : (r.frag == FragKind::h3t ? c.h3t : -1)));
    const float* wfrag = foff >= 0 ? b.dv.wpack + foff : nullptr;
    int rc;
    { ProfScope ps(e, r.cls, geom_macs(g), s); rc = conv_launch(r, g, x, gate, w, wfrag, bias, skip, y, am, s); }
    if (rc == PROBAV_OK && am.y && !r.reports) rc = amax_tensor(y, (size_t)g.Ho * g.Wo * g.To * g.Cout, g.N, am.y, s);
    return rc;
}
static int conv_wgrad(const PassBufs& b, const Launch& L, const float* x, const float* dy, const float* gate, const Amax& am, hipStream_t s)
{
    const probav_engine* e = b.e;
    const ConvGeom& g = L.g;
    CK(operands_agree(L, LaunchKind::wgrad, gate, nullptr, am));
    const WgradRoute r = wgrad_route(e->fam, g, L.o);
    if (wgrad_slab_floats(r, g) > L.slab.floats) { set_error("probav_backward: a backward-filter launch needs a larger slab region than make_plan laid out", hipSuccess); return PROBAV_EINVAL; }
    if (census_slot(r) >= 0) ++const_cast<probav_engine*>(e)->launched[census_slot(r)];
    const WnLayer& wn = e->layers[L.li].wn;
    float *dw = b.dweff2 + wn.w_off, *db = b.grads + wn.b_off, *part = b.slabs + L.slab.off;
    ProfScope ps(e, r.cls, geom_macs(g), s);
    switch (r.k) {
    case WgradKernel::x6: return x6_conv_wgrad(g, x, dy, gate, dw, db, part, r.arith, am, s);
    case WgradKernel::mfma: return mfma_conv_wgrad(g, x, dy, gate, dw, db, part, s);
    case WgradKernel::gemm: return r.wide ? gemm_conv_wgrad_wide(g, x, dy, gate, dw, db, part, s) : gemm_conv_wgrad(g, x, dy, gate, dw, db, part, s);
    default: return conv3d_direct_wgrad(g, x, dy, gate, dw, db, part, s);
    }
}

// What gets packed into MFMA operand fragments: a 3x3x3 filter (of either direction), the per-tap H3 form of a 25-channel one (the piece-ring
// strip kernel's operand order; the other forms of 25 channels are K-concatenated), and the fused pointwise pair's W1, W2 (forward) and
// W2, W1 as the operands of its backward
enum class Operand { conv, conv_taps, pw_w1, pw_w2, pw_w2b, pw_w1c };
// a filled packing job for `op` of a cin x cout matrix (conv: of the packed direction) in arithmetic `arith` (0 fp32, 1 X6, 2 H3); the caller
// sets src_off, dst_off, src_is_T and amax_slot.  count == 0: the fp32 MFMA kernels have no fragments for this channel configuration
static PackJob pack_job(Operand op, int arith, int cin, int cout)
{
    PackJob J; memset(&J, 0, sizeof(J));
    if (op == Operand::conv || op == Operand::conv_taps) {
        if (arith == 0) { mfma_conv_pack_job(J, cin, cout); return J; }
        const bool kc = cin == 25;
        J.Cin = cin; J.Cout = cout; J.taps = 27;
        if (arith == 1) { J.type = kc ? PACK_X6_CONVK : PACK_X6_CONV; J.count = kc ? X6_CONVK_FRAG_WORDS : X6_CONV_FRAG_WORDS; return J; }
        J.type = kc ? (op == Operand::conv_taps ? PACK_H3_CONVP : PACK_H3_CONVK) : PACK_H3_CONV;
        J.count = kc ? H3_CONVK_FRAG_WORDS : H3_CONV_FRAG_WORDS;
        J.amax_percol = 1; J.ncol = cout;                      // H3: cut per output column of the packed matrix
        return J;
    }
    static const int types[3][4] = {{PACK_PW_A_KCIN, PACK_PW_A_KHCH, PACK_PW_A_KOUT, PACK_PW_A_CIN_KHCH},
                                    {PACK_X6_PW_W1, PACK_X6_PW_W2, PACK_X6_PW_W2K, PACK_X6_PW_W1C},
                                    {PACK_H3_PW_W1, PACK_H3_PW_W2, PACK_H3_PW_W2K, PACK_H3_PW_W1C}};
    J.type = types[arith][(int)op - (int)Operand::pw_w1];
    J.count = arith == 0 ? 8 * 4 * 64 * 4 : (arith == 1 ? X6_PW_FRAG_WORDS : H3_PW_FRAG_WORDS);
    J.Cin = cin; J.Cout = cout;
    // H3: W2 forward is cut per output column d, W1 as the operand of (c) per cin row (= dX column); the other two take one scale for the tensor
    if (arith == 2 && op == Operand::pw_w2) { J.amax_percol = 1; J.ncol = cout; }
    if (arith == 2 && op == Operand::pw_w1c) { J.amax_percol = 1; J.ncol = cin; }
    return J;
}

// the fused pointwise pair (expConv + ReLU + decConv), one launch each way: the fp32-MFMA kernels (arith 0) or the split-operand ones (1 X6, 2 H3)
struct PwOps { const float *w1, *w2, *w2b, *w1c; };
static int pw_forward(int arith, const PwOps& f, const float* x, const float* b1, const float* b2, float* dec, long nvox, long vps, int D,
                      const PwAmax& am, hipStream_t s, float* hidden = nullptr)
{
    if (arith) return x6_pw_forward(x, f.w1, f.w2, b1, b2, dec, nvox, vps, D, arith, am, s, hidden);
    return mfma_pw_forward(x, f.w1, f.w2, b1, b2, dec, nvox, D, s);
}
static int pw_backward(int arith, const PwOps& f, const float* x, const float* dT, const float* dOut, const float* b1, float* dX, float* dW1,
                       float* dW2, float* db1, float* db2, float* slabs, long nvox, long vps, int D, const PwAmax& am, hipStream_t s)
{
    if (arith) return x6_pw_backward(x, dT, dOut, f.w1, f.w2b, f.w1c, b1, dX, dW1, dW2, db1, db2, slabs, nvox, vps, D, arith, am, s);
    return mfma_pw_backward(x, dT, dOut, f.w1, f.w2b, f.w1c, b1, dX, dW1, dW2, db1, db2, slabs, nvox, D, s);
}
// block i's pair in the engine's family: its fragments (in the packed region `wpack`) and, H3, its amax slots
static PwOps block_frags(const probav_engine* e, const float* wpack, int i)
{
    const PwFrags& o = e->pkBlk[i][e->fam.arith];
    return {wpack + o.w1, wpack + o.w2, wpack + o.w2b, wpack + o.w1c};
}
// forward of block i from act[i] (x) into dec; ay: per-sample slots of the output's amax (H3, optional); hidden: test dump of the hidden tile
static int pw_forward_launch(const probav_engine* e, int i, const float* wpack, const AmaxSlots& A, const float* params, const float* x,
                             float* dec, long nvox, unsigned* ay, hipStream_t s, float* hidden = nullptr)
{
    const int le = e->iExp[i], ld = e->iDec[i];
    PwAmax m;
    if (e->fam.arith == 2) { m.x = A.act(i); m.w1 = A.w(le); m.w2 = A.w(ld); m.w2c = A.wcol(ld); m.b1 = A.b(le); m.y = ay; }
    return pw_forward(e->fam.arith, block_frags(e, wpack, i), x, params + e->layers[le].wn.b_off, params + e->layers[ld].wn.b_off, dec,
                      nvox, nvox / A.B, e->cfg.dec_channels, m, s, hidden);
}
// backward of block i: dT = d loss / d dec_i, dOut = d loss / d act[i+1] (the skip path) -> dX, the weight (into dweff2) and bias (into grads)
// gradients of expConv_i and decConv_i; adt / ay: amax slots of dT / dX (H3)
static int pw_backward_launch(const PassBufs& b, const Launch& L, const AmaxSlots& A, const float* x, const float* dT, const float* dOut, float* dX,
                              unsigned* adt, unsigned* ay, hipStream_t s)
{
    const probav_engine* e = b.e;
    const int i = L.i, D = e->cfg.dec_channels;
    const long nvox = in_voxels(L.g);
    if (L.kind != LaunchKind::fused || mfma_pw_backward_slab_floats(D) > L.slab.floats) { set_error("probav_backward: the fused pointwise pair's launch is not in the launch list, or its slab region is too small", hipSuccess); return PROBAV_EINVAL; }
    const WnLayer &we = e->layers[e->iExp[i]].wn, &wd = e->layers[e->iDec[i]].wn;
    PwAmax m;
    if (e->fam.arith == 2) { m.x = A.act(i); m.w1 = A.w(e->iExp[i]); m.w2 = A.w(e->iDec[i]); m.w1r = A.wrow(e->iExp[i]); m.b1 = A.b(e->iExp[i]); m.dt = adt; m.y = ay; }
    return pw_backward(e->fam.arith, block_frags(e, b.dv.wpack, i), x, dT, dOut, b.params + we.b_off, dX, b.dweff2 + we.w_off, b.dweff2 + wd.w_off,
                       b.grads + we.b_off, b.grads + wd.b_off, b.slabs + L.slab.off, nvox, nvox / A.B, D, m, s);
}

// the general matrix route's pair (kernels_gemm_pw.hip) of block i: the effective weights as the route's other launches read them.  It does not report amax: where the
// launch list's neighbours are H3 kernels, ay (per-sample slots of the output) is filled by amax_tensor behind the launch, as conv_fwd does for the route
static int gemm_pair_forward_launch(const probav_engine* e, int i, const Derived& dv, const float* params, const float* x, float* dec, const ConvGeom& g,
                                    unsigned* ay, hipStream_t s, float* hidden = nullptr)
{
    const WnLayer &we = e->layers[e->iExp[i]].wn, &wd = e->layers[e->iDec[i]].wn;
    const int D = e->cfg.dec_channels;
    CK(gemm_pw_forward(x, dv.weff + we.w_off, params + we.b_off, dv.weff + wd.w_off, params + wd.b_off, dec, hidden, in_voxels(g), g.Cin, g.Cout, D, s));
    if (ay) CK(amax_tensor(dec, (size_t)g.Ho * g.Wo * g.To * D, g.N, ay, s));
    return PROBAV_OK;
}
static int gemm_pair_backward_launch(const PassBufs& b, const Launch& L, const float* x, const float* dT, const float* dOut, float* dX, unsigned* ay, hipStream_t s)
{
    const probav_engine* e = b.e;
    const ConvGeom& g = L.g;
    const int i = L.i, D = e->cfg.dec_channels;
    if (L.kind != LaunchKind::fused || gemm_pw_backward_slab_floats(g.Cin, g.Cout, D, in_voxels(g)) > L.slab.floats) { set_error("probav_backward: the general fused pointwise pair's launch is not in the launch list, or its slab region is too small", hipSuccess); return PROBAV_EINVAL; }
    const WnLayer &we = e->layers[e->iExp[i]].wn, &wd = e->layers[e->iDec[i]].wn;
    CK(gemm_pw_backward(x, dT, dOut, b.dv.weff + we.w_off, b.params + we.b_off, b.dv.weff + wd.w_off, dX, b.dweff2 + we.w_off, b.dweff2 + wd.w_off,
                        b.grads + we.b_off, b.grads + wd.b_off, b.slabs + L.slab.off, in_voxels(g), g.Cin, g.Cout, D, s));
    if (ay) CK(amax_tensor(dX, (size_t)g.Hi * g.Wi * g.Ti * g.Cin, g.N, ay, s));
    return PROBAV_OK;
}

extern "C" {

int probav_abi_version(void) { return PROBAV_ABI_VERSION; }
int probav_engine_side_stream(probav_engine* e, int mode)
{
    if (!e || mode < 0 || mode > 2) { set_error("probav_engine_side_stream: bad argument", hipSuccess); return PROBAV_EINVAL; }
    e->side_mode = mode;
    return PROBAV_OK;
}
int probav_mfma_probe(const void* seed, float* sink, int iters, int launches, void* stream)
{
    if (!seed || !sink || iters < 1 || launches < 1) { set_error("probav_mfma_probe: null/invalid argument", hipSuccess); return PROBAV_EINVAL; }
    return mfma_probe(seed, sink, iters, launches, (hipStream_t)stream);
}
int probav_mfma_probe_shape(const void* seed, float* sink, int iters, int launches, int shape, void* stream)
{
    if (!seed || !sink || iters < 1 || launches < 1 || shape < 0 || shape > 1) { set_error("probav_mfma_probe_shape: null/invalid argument", hipSuccess); return PROBAV_EINVAL; }
    return mfma_probe(seed, sink, iters, launches, (hipStream_t)stream, shape);
}
const char* probav_last_error(void) { return probav::last_error(); }

int probav_engine_create(const probav_net_cfg* cfg, probav_engine** out)
{
    if (!cfg || !out) { set_error("probav_engine_create: null argument", hipSuccess); return PROBAV_EINVAL; }
    const int T = cfg->num_img_lr;
    if (cfg->scale != 3 || cfg->max_shift != 2 * cfg->scale) {
        set_error("probav_engine_create: the reference graph only closes for scale=3, maxShift=6 (models/modelsTF.py:45-53)", hipSuccess);
        return PROBAV_EINVAL;
    }
    if (T != 7 && T != 9 && T != 13 && T != 19) {
        set_error("probav_engine_create: numImgLR must be 7, 9, 13 or 19 (models/modelsTF.py:62-69)", hipSuccess);
        return PROBAV_EINVAL;
    }
    if (cfg->num_filters < 1 || cfg->num_res_blocks < 0 || cfg->exp_rate < 1 || cfg->dec_channels < 1 ||
        cfg->patch_size_lr < 1 || !(cfg->std > 0.f) || (cfg->in_channels != 1 && cfg->in_channels != 3)) {
        set_error("probav_engine_create: bad hyper-parameter", hipSuccess);
        return PROBAV_EINVAL;
    }
    probav_engine* e = new probav_engine();
    e->cfg = *cfg;
    e->Hin = cfg->patch_size_lr + cfg->max_shift;
    const int F = cfg->num_filters, E = F * cfg->exp_rate, D = cfg->dec_channels, s2 = cfg->scale * cfg->scale;
    const int Cx = cfg->in_channels;                                   // 1, or 3 for isGrayScale=False (models/modelsTF.py:19-20)
    e->iMain = add_layer(e, "mainConv1", 3, 3, 3, Cx, F);
    for (int i = 0; i < cfg->num_res_blocks; ++i) {
        e->iExp.push_back(add_layer(e, "expConv_" + std::to_string(i), 1, 1, 1, F, E));
        e->iDec.push_back(add_layer(e, "decConv_" + std::to_string(i), 1, 1, 1, E, D));
        e->iNorm.push_back(add_layer(e, "normConv_" + std::to_string(i), 3, 3, 3, D, F));
    }
    typedef probav_engine::RedSpec RS;
    if (T == 9) e->redSpec = {RS{3, 1, 0, 1, 0}, RS{3, 0, 0, 0, 0}, RS{3, 0, 0, 0, 0}};
    else if (T == 13) e->redSpec = {RS{3, 1, 0, 1, 0}, RS{3, 1, 0, 1, 0}, RS{3, 1, 0, 1, 0}, RS{3, 0, 0, 0, 0}, RS{3, 0, 0, 0, 0}};
    else if (T == 7) e->redSpec = {RS{3, 0, 0, 0, 0}, RS{3, 0, 0, 0, 0}};
    else   // T == 19, ConvReduceAndUpscaleEx (models/modelsTF.py:76-121, marked EXPERIMENTAL there): a 5x5x5 layer on a fully mirrored pad of 2,
           // four 3x3x3 layers on mirrored H/W pads of 2, 2, 2, 1 (the first also mirrors one frame of depth), five plain valid ones
        e->redSpec = {RS{5, 2, 2, 1, 1}, RS{3, 2, 1, 1, 1}, RS{3, 2, 0, 1, 0}, RS{3, 2, 0, 1, 0}, RS{3, 1, 0, 1, 0},
                      RS{3, 0, 0, 0, 0}, RS{3, 0, 0, 0, 0}, RS{3, 0, 0, 0, 0}, RS{3, 0, 0, 0, 0}, RS{3, 0, 0, 0, 0}};
    for (size_t k = 0; k < e->redSpec.size(); ++k)
        e->iRed.push_back(add_layer(e, "convReducer_" + std::to_string(k + 1), e->redSpec[k].k, e->redSpec[k].k, e->redSpec[k].k, F, F));
    e->iResid1 = add_layer(e, "residConv1", 3, 3, 1, Cx, s2);
    e->iUp = add_layer(e, "upscaleConv1", 3, 3, 3, F, s2);
    e->iResid2 = add_layer(e, "residConv2", 3, 3, 1, s2, s2);
    e->iResid3 = add_layer(e, "residConv3", 3, 3, 1, s2, s2);
    // the graph must close: after the reducers one valid 3x3x3 conv lands on [P, P, 1]
    const ConvGeom up = make_net(e, 1).up;
    if (up.Hi - 2 != up.Ho || up.Ti - 2 != up.To) {
        delete e;
        set_error("probav_engine_create: reducer geometry does not collapse to [P,P,1]", hipSuccess);
        return PROBAV_EINVAL;
    }
    // MFMA fragment-packing jobs: every family's fragments, packed whenever weights are normalised at impl >= 1
    const int L2 = 2 * (int)e->layers.size();                      // weight amax slots per column of weff, then per column of weffT (wn_forward's layout)
    auto add = [&](PackJob J, long src_off, int src_is_T, int amax_slot) -> long {
        J.src_off = src_off; J.src_is_T = src_is_T; J.amax_slot = amax_slot; J.dst_off = e->wpack_count;
        e->wpack_count += J.count;
        e->jobs.push_back(J);
        return J.dst_off;
    };
    for (size_t li = 0; li < e->layers.size(); ++li) {
        LayerRec& r = e->layers[li];
        if (r.kh != 3 || r.kw != 3 || r.kt != 3) continue;
        for (int dir = 0; dir < 2; ++dir) {
            const int cin = dir ? r.wn.Cout : r.wn.Cin, cout = dir ? r.wn.Cin : r.wn.Cout;
            if ((int)li == e->iMain && dir) continue;               // input-facing: no backward-data
            const PackJob J = pack_job(Operand::conv, 0, cin, cout);
            if (J.count == 0) continue;
            ConvFrags& o = r.pk[dir];
            o.f32 = add(J, r.wn.w_off, dir, 0);
            if ((cin == 25 || cin == 32) && cout <= 32) {           // strip-kernel shapes: also the split-operand fragments
                const int wcols = L2 + (dir ? (int)e->cout_total + r.wn.r_off : r.wn.n_off);   // H3: the packed matrix' columns
                o.x6 = add(pack_job(Operand::conv, 1, cin, cout), r.wn.w_off, dir, 0);
                o.h3 = add(pack_job(Operand::conv, 2, cin, cout), r.wn.w_off, dir, wcols);
                if (cin == 25) o.h3t = add(pack_job(Operand::conv_taps, 2, cin, cout), r.wn.w_off, dir, wcols);
            }
        }
    }
    e->pw_mfma = mfma_pw_supported(F, E, D);
    for (int i = 0; e->pw_mfma && i < cfg->num_res_blocks; ++i) {
        const int le = e->iExp[i], ld = e->iDec[i];
        const long w1 = e->layers[le].wn.w_off, w2 = e->layers[ld].wn.w_off;
        std::array<PwFrags, 3> b;
        for (int a = 0; a < 2; ++a) {                               // fp32, X6: no amax
            b[a].w1 = add(pack_job(Operand::pw_w1, a, F, E), w1, 0, 0);
            b[a].w2 = add(pack_job(Operand::pw_w2, a, E, D), w2, 0, 0);
            b[a].w2b = add(pack_job(Operand::pw_w2b, a, E, D), w2, 0, 0);
            b[a].w1c = add(pack_job(Operand::pw_w1c, a, F, E), w1, 0, 0);
        }
        // H3 (in this order): W1 and W2-backward scaled by their tensors' slots, W1-backward per cin row, W2 per output column
        b[2].w1 = add(pack_job(Operand::pw_w1, 2, F, E), w1, 0, le);
        b[2].w1c = add(pack_job(Operand::pw_w1c, 2, F, E), w1, 0, L2 + (int)e->cout_total + e->layers[le].wn.r_off);
        b[2].w2 = add(pack_job(Operand::pw_w2, 2, E, D), w2, 0, L2 + e->layers[ld].wn.n_off);
        b[2].w2b = add(pack_job(Operand::pw_w2b, 2, E, D), w2, 0, ld);
        e->pkBlk.push_back(b);
    }
    // (the layer and packing tables go to the device with the first call that launches with them: device_tables)
    const char* env = getenv("PROBAV_IMPL");
    const char* genv = getenv("PROBAV_GEMM_ROUTE");                // set and non-zero: the general matrix route is on from the start
    const char* penv = getenv("PROBAV_GEMM_PAIR");                 // set and non-zero: the wish for the route's fused pointwise pair is on from the start
    e->impl = env ? atoi(env) : 4;
    e->gemm = genv && atoi(genv) != 0;
    e->gemm_pair = penv && atoi(penv) != 0;
    const char* xenv = getenv("PROBAV_GEMM_X6");                   // set and non-zero: the wish for the route's x6 arithmetic is on from the start
    e->gemm_x6 = xenv && atoi(xenv) != 0;
    const char* eenv = getenv("PROBAV_GEMM_EXOTIC");               // set and non-zero: the wish for the route's exotic launches is on from the start
    e->gemm_exotic = eenv && atoi(eenv) != 0;
    e->pw_gemm = gemm_pw_supported(F, E, D, (long)e->Hin * e->Hin * T);
    e->fam = engine_family(e);
    *out = e;
    return PROBAV_OK;
}

// The layer table and the packing jobs on the device, uploaded by the first call that launches with them (like the side stream, created on the engine's
// first pass: make that call outside a graph capture).  probav_engine_create itself touches no device, so the size and layout queries of a configuration
// answer on a host without one.
static int device_tables(probav_engine* e)
{
    if (e->d_layers) return PROBAV_OK;
    if (!e->jobs.empty() && !e->d_jobs) {
        hipError_t perr = hipMalloc((void**)&e->d_jobs, e->jobs.size() * sizeof(PackJob));
        if (perr == hipSuccess) perr = hipMemcpy(e->d_jobs, e->jobs.data(), e->jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice);
        if (perr != hipSuccess) { if (e->d_jobs) (void)hipFree(e->d_jobs); e->d_jobs = nullptr; set_error("probav_engine: pack table upload", perr); return PROBAV_EHIP; }
    }
    std::vector<WnLayer> h;
    for (auto& r : e->layers) h.push_back(r.wn);
    WnLayer* d = nullptr;
    hipError_t err = hipMalloc((void**)&d, h.size() * sizeof(WnLayer));
    if (err == hipSuccess) err = hipMemcpy(d, h.data(), h.size() * sizeof(WnLayer), hipMemcpyHostToDevice);
    if (err != hipSuccess) { if (d) (void)hipFree(d); set_error("probav_engine: layer table upload", err); return PROBAV_EHIP; }
    e->d_layers = d;
    return PROBAV_OK;
}

int probav_engine_profile(probav_engine* e, int enable, int max_launches)
{
    if (!e || max_launches < 0) { set_error("probav_engine_profile: bad argument", hipSuccess); return PROBAV_EINVAL; }
    while ((int)e->prof_ev.size() < 2 * max_launches) {
        hipEvent_t ev;
        hipError_t err = hipEventCreate(&ev);
        if (err != hipSuccess) { set_error("probav_engine_profile: hipEventCreate", err); return PROBAV_EHIP; }
        e->prof_ev.push_back(ev);
    }
    e->prof_on = enable != 0;
    e->prof_used = 0; e->prof_cls.clear(); e->prof_macs.clear();
    return PROBAV_OK;
}

int probav_engine_profile_classes(probav_engine* e, uint32_t mask)
{
    if (!e) { set_error("probav_engine_profile_classes: null engine", hipSuccess); return PROBAV_EINVAL; }
    e->prof_mask = mask;
    return PROBAV_OK;
}

int probav_engine_profile_read(probav_engine* e, int nclass, double* ms, double* macs, int64_t* launches)
{
    if (!e || !ms || !macs || !launches || nclass < CLS_COUNT) { set_error("probav_engine_profile_read: bad argument", hipSuccess); return PROBAV_EINVAL; }
    for (int c = 0; c < nclass; ++c) { ms[c] = 0; macs[c] = 0; launches[c] = 0; }
    for (size_t i = 0; i < e->prof_cls.size(); ++i) {
        float t = 0.f;
        hipError_t err = hipEventElapsedTime(&t, e->prof_ev[2 * i], e->prof_ev[2 * i + 1]);     // caller has synchronised
        if (err != hipSuccess) { set_error("probav_engine_profile_read: hipEventElapsedTime", err); return PROBAV_EHIP; }
        const int c = e->prof_cls[i];
        ms[c] += t; macs[c] += e->prof_macs[i]; launches[c] += 1;
    }
    e->prof_used = 0; e->prof_cls.clear(); e->prof_macs.clear();
    return PROBAV_OK;
}

void probav_engine_destroy(probav_engine* e)
{
    if (!e) return;
    for (auto ev : e->prof_ev) (void)hipEventDestroy(ev);
    reduce_free_pending(&e->side);
    if (e->side.side) {
        (void)hipStreamSynchronize(e->side.side);
        for (auto ev : e->side.ev) (void)hipEventDestroy(ev);
        (void)hipEventDestroy(e->side.joined);
        (void)hipStreamDestroy(e->side.side);
    }
    if (e->d_layers) (void)hipFree(e->d_layers);
    if (e->d_jobs) (void)hipFree(e->d_jobs);
    delete e;
}

int64_t probav_param_count(const probav_engine* e) { return e ? e->nparams : -1; }
int probav_num_layers(const probav_engine* e) { return e ? (int)e->layers.size() : -1; }
int64_t probav_weff_count(const probav_engine* e) { return e ? e->weff_count : -1; }
int64_t probav_cout_total(const probav_engine* e) { return e ? e->cout_total : -1; }

int probav_layer_info(const probav_engine* e, int i, char name[32], int64_t* g_off, int64_t* v_off, int64_t* b_off, int32_t shape[5])
{
    if (!e || i < 0 || i >= (int)e->layers.size()) { set_error("probav_layer_info: bad index", hipSuccess); return PROBAV_EINVAL; }
    const LayerRec& r = e->layers[i];
    if (name) memcpy(name, r.name, 32);
    if (g_off) *g_off = r.wn.g_off;
    if (v_off) *v_off = r.wn.v_off;
    if (b_off) *b_off = r.wn.b_off;
    if (shape) { shape[0] = r.kh; shape[1] = r.kw; shape[2] = r.kt; shape[3] = r.wn.Cin; shape[4] = r.wn.Cout; }
    return PROBAV_OK;
}

int probav_engine_set_impl(probav_engine* e, int impl)
{
    if (!e || impl < 0 || impl > 4) { set_error("probav_engine_set_impl: bad argument", hipSuccess); return PROBAV_EINVAL; }
    e->impl = impl;
    e->fam = engine_family(e);
    return PROBAV_OK;
}

int probav_engine_set_gemm_route(probav_engine* e, int on)
{
    if (!e) { set_error("probav_engine_set_gemm_route: null engine", hipSuccess); return PROBAV_EINVAL; }
    e->gemm = on != 0;
    e->fam = engine_family(e);
    return PROBAV_OK;
}
int probav_engine_gemm_route(const probav_engine* e) { return e && e->gemm ? 1 : 0; }

int probav_engine_set_gemm_pair(probav_engine* e, int on)
{
    if (!e) { set_error("probav_engine_set_gemm_pair: null engine", hipSuccess); return PROBAV_EINVAL; }
    e->gemm_pair = on != 0;
    e->fam = engine_family(e);
    return PROBAV_OK;
}
int probav_engine_gemm_pair(const probav_engine* e) { return e && e->gemm_pair ? 1 : 0; }
int probav_engine_pair_kind(const probav_engine* e) { return e ? (int)e->fam.pw_fused : 0; }

int probav_engine_set_gemm_x6(probav_engine* e, int on)
{
    if (!e) { set_error("probav_engine_set_gemm_x6: null engine", hipSuccess); return PROBAV_EINVAL; }
    e->gemm_x6 = on != 0;
    e->fam = engine_family(e);
    return PROBAV_OK;
}
int probav_engine_gemm_x6(const probav_engine* e) { return e && e->gemm_x6 ? 1 : 0; }
int probav_engine_gemm_arith(const probav_engine* e) { return e ? e->fam.gemm_arith : 0; }

int probav_engine_set_gemm_exotic(probav_engine* e, int on)
{
    if (!e) { set_error("probav_engine_set_gemm_exotic: null engine", hipSuccess); return PROBAV_EINVAL; }
    e->gemm_exotic = on != 0;
    e->fam = engine_family(e);
    return PROBAV_OK;
}
int probav_engine_gemm_exotic(const probav_engine* e) { return e && e->gemm_exotic ? 1 : 0; }

int probav_plan_pw_gemm(int F, int H, int D, int64_t nvox, int backward, int32_t report[8])
{
    if (!report) { set_error("probav_plan_pw_gemm: null report", hipSuccess); return PROBAV_EINVAL; }
    int v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (!gemm_pw_plan_ints(F, H, D, (long)nvox, backward != 0, v)) for (int i = 0; i < 8; ++i) v[i] = 0;
    for (int i = 0; i < 8; ++i) report[i] = v[i];
    return PROBAV_OK;
}

size_t probav_workspace_bytes(const probav_engine* e, int batch, int training)
{
    if (!e || batch < 1) return 0;
    return make_plan(e, batch, training).total * sizeof(float);
}

static ReduceSide* engine_side(probav_engine* e)
{
    if (!e->side_tried) {
        e->side_tried = true;
        ReduceSide c = {};
        // lowest priority: its kernels are fillers for the gaps of the caller's chain, never competitors
        int prio_least = 0, prio_greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) { (void)hipGetLastError(); prio_least = 0; }
        bool ok = hipStreamCreateWithPriority(&c.side, hipStreamNonBlocking, prio_least) == hipSuccess;
        for (int i = 0; ok && i < 8; ++i) ok = hipEventCreateWithFlags(&c.ev[i], hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&c.joined, hipEventDisableTiming) == hipSuccess;
        if (ok) e->side = c; else (void)hipGetLastError();          // (without it the sums simply stay on the caller's stream)
    }
    return e->side.side ? &e->side : nullptr;
}

struct SideGuard {          // activates the engine's side stream (probav_common.h: ReduceSide) for the calling thread while a pass is being enqueued
    ReduceSide* c;
    hipStream_t s;
    SideGuard(ReduceSide* c_, hipStream_t s_, int defer = 0) : c(c_), s(s_) { if (c) { c->k = 0; c->last = nullptr; c->defer = defer; reduce_side_activate(c); reduce_drop_pending(); } }
    ~SideGuard()
    {
        if (!c) return;
        reduce_drop_pending();                      // (a pass that returned early: queued launches may point into its frame -- never run them here)
        if (c->k != 0) (void)reduce_join(s);        // a pass that returned early (an error): whatever was forked still rejoins the caller's stream
        c->defer = 0;
        reduce_side_activate(nullptr);
    }
};
static bool side_stream_disabled() { static const bool v = getenv("PROBAV_NO_SIDE_STREAM") != nullptr; return v; }   // diagnostic: everything on the caller's stream

static int forward_impl(probav_engine* e, const float* params, const float* x, float* y, void* ws, size_t ws_bytes,
                        int B, int training, const float* WC, void* stream)
{
    if (!e || !params || !x || !y || !ws || B < 1) { set_error("probav_forward: null/invalid argument", hipSuccess); return PROBAV_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const Plan p = make_plan(e, B, training);
    if (ws_bytes < p.fwd_total * sizeof(float)) { set_error("probav_forward: workspace too small", hipSuccess); return PROBAV_ENOSPACE; }
    CK(device_tables(e));
    float* W = (float*)ws;
    const Net& n = p.net;
    const Derived dv = derived(e, p, W, WC);
    const probav_net_cfg& c = e->cfg;
    const int R = c.num_res_blocks;
    auto weff = [&](int li) { return dv.weff + e->layers[li].wn.w_off; };
    auto bias = [&](int li) { return params + e->layers[li].wn.b_off; };
    const PassBufs pb = {e, dv, params, nullptr, nullptr, nullptr};
    auto fwd = [&](Role role, int i = 0) { return launch_at(p, role, LaunchKind::conv, false, i); };
    // amax slots (H3 arithmetic, impl 4): every tensor an H3 kernel reads has its largest magnitude in a slot by then
    const bool h3 = e->fam.arith == 2;
    const AmaxSlots A(e, p, W, dv.wslots);
    auto amx = [&](const unsigned* ax, int li, unsigned* ay) { Amax m; if (h3) { m.x = ax; m.w = A.wcol(li); m.y = ay; } return m; };
    // (the per-sample amax slots -- the atomicMax targets -- are cleared by head_kernel below; the weight slots in front of them are plain stores of wn_forward_kernel /
    // wn_rowmax_kernel, every one of them written before anything reads it)
    if (training) { e->fwd_amax = h3; e->fwd_pair = e->fam.pw_fused; e->fwd_gemm_arith = e->fam.gemm_arith; e->fwd_gemm_exotic = e->fam.gemm_exotic; }

    if (!WC) {
        { ProfScope ps(e, CLS_WN, 0.0, s); CK(wn_forward(e->d_layers, (int)e->layers.size(), (int)e->cout_total, (int)e->cin_total, params, W + p.weff, W + p.weffT, W + p.invn, h3 ? A.base : nullptr, s)); }
        if (e->fam.mfma) { ProfScope ps(e, CLS_WN, 0.0, s); CK(mfma_pack(e->d_jobs, (int)e->jobs.size(), W + p.weff, W + p.weffT, W + p.wpack, A.base, s)); }
    }
    CK(head_forward(x, W + p.xn, W + p.mn, B * n.main.Hi * n.main.Wi, n.main.Ti, n.main.Cin, c.mean, c.std, s, h3 ? A.base + p.amax_fwd : nullptr, h3 ? p.amax_bwd - p.amax_fwd : 0));
    // the low-frequency residual path (three small 2-D convolutions on the temporal mean) meets the main path only in tail_forward: it runs
    // on the side stream, in the gaps of the chip-filling launches
    SideGuard side_guard((side_stream_disabled() || e->side_mode == 0) ? nullptr : engine_side(e), s);
    {
        hipStream_t rs = reduce_fork(s);
        const Launch path = launch_at(p, Role::resid_path, LaunchKind::fused, false);
        if (path.kind == LaunchKind::fused) {              // the three layers as one launch (kernels_direct.hip); family 0 keeps the generic direct kernels
            CK(resid_path_forward(B, path.g.Hi, path.g.Cin, W + p.mn, weff(e->iResid1), bias(e->iResid1), weff(e->iResid2), bias(e->iResid2), weff(e->iResid3), bias(e->iResid3),
                                  W + p.r1, W + p.r2, W + p.r3, rs));
        } else {
        CK(conv_fwd(pb, fwd(Role::resid1), W + p.mn, nullptr, nullptr, W + p.r1, Amax(), rs));
        CK(conv_fwd(pb, fwd(Role::resid2), W + p.r1, nullptr, nullptr, W + p.r2, Amax(), rs));
        CK(conv_fwd(pb, fwd(Role::resid3), W + p.r2, nullptr, nullptr, W + p.r3, Amax(), rs));
        }
    }
    CK(conv_fwd(pb, fwd(Role::main), W + p.xn, nullptr, nullptr, W + p.act[0], amx(nullptr, e->iMain, A.act(0)), s));
    for (int i = 0; i < R; ++i) {
        const Launch pair = launch_at(p, Role::pair, LaunchKind::fused, false, i);
        if (pair.kind == LaunchKind::fused && e->fam.pw_fused == PairKind::gemm) {
            // the general matrix route's pair: any channel counts, the route's operands (fp32 class, the pair's algorithmic MACs)
            ProfScope ps(e, CLS_PW_FWD, geom_macs(n.exp) + geom_macs(n.dec), s);
            CK(gemm_pair_forward_launch(e, i, dv, params, W + p.act[i], W + p.dec[i], pair.g, h3 ? A.dec(i) : nullptr, s));
        } else if (pair.kind == LaunchKind::fused) {
            // fused expConv + ReLU + decConv: the 256-channel tensor never leaves the accumulators
            ProfScope ps(e, e->fam.x6 ? CLS_PW_FWD_X6 : CLS_PW_FWD, geom_macs(n.exp) + geom_macs(n.dec), s);
            CK(pw_forward_launch(e, i, dv.wpack, A, params, W + p.act[i], W + p.dec[i], in_voxels(pair.g), A.dec(i), s));
        } else {
            CK(conv_fwd(pb, fwd(Role::exp, i), W + p.act[i], nullptr, nullptr, W + p.H, Amax(), s));
            CK(conv_fwd(pb, fwd(Role::dec, i), W + p.H, nullptr, nullptr, W + p.dec[i], amx(nullptr, e->iDec[i], A.dec(i)), s));
        }
        CK(conv_fwd(pb, fwd(Role::norm, i), W + p.dec[i], nullptr, W + p.act[i], W + p.act[i + 1], amx(A.dec(i), e->iNorm[i], A.act(i + 1)), s));
    }
    const float* cur = W + p.act[R];
    const unsigned* acur = A.act(R);
    for (int k = 0; k < (int)n.red.size(); ++k) {
        CK(conv_fwd(pb, fwd(Role::red, k), cur, nullptr, nullptr, W + p.red[k], amx(acur, e->iRed[k], A.red(k)), s));
        cur = W + p.red[k]; acur = A.red(k);
    }
    CK(conv_fwd(pb, fwd(Role::up), cur, nullptr, nullptr, W + p.up, amx(acur, e->iUp, nullptr), s));
    CK(reduce_join(s));                                                       // the residual path has arrived
    CK(tail_forward(W + p.up, W + p.r3, y, B, n.up.Ho, c.scale, c.mean, c.std, s));
    return PROBAV_OK;
}

int probav_forward(probav_engine* e, const float* params, const float* x, float* y, void* ws, size_t ws_bytes,
                   int B, int training, void* stream)
{
    return forward_impl(e, params, x, y, ws, ws_bytes, B, training, nullptr, stream);
}
int probav_forward_wc(probav_engine* e, const float* params, const float* x, float* y, void* ws, size_t ws_bytes,
                      int B, int training, const void* wcache, size_t wcache_bytes, void* stream)
{
    if (!e || !wcache) { set_error("probav_forward_wc: null engine / weight cache", hipSuccess); return PROBAV_EINVAL; }
    if (wcache_bytes < make_wc_plan(e).total * sizeof(float)) { set_error("probav_forward_wc: weight cache too small", hipSuccess); return PROBAV_ENOSPACE; }
    return forward_impl(e, params, x, y, ws, ws_bytes, B, training, (const float*)wcache, stream);
}

// ws: the saved state of the matching forward pass (READ ONLY here); scratch: what the reverse pass writes on its way (gradient buffers, slabs, its amax
// slots; contents meaningless before and after).  scratch == nullptr: the one-piece form, the scratch is the tail of `ws`.
// dx (optional): d loss / d x, one more launch at the end of the pass (kernels_input_grad.hip); null: the pass issues the launches and writes the bits it always did
static int backward_impl(probav_engine* e, const float* params, const float* dy, float* grads, const void* ws, size_t ws_bytes,
                         void* scratch, size_t scratch_bytes, int B, const float* WC, void* stream, float* dx = nullptr)
{
    if (!e || !params || !dy || !grads || !ws || B < 1) { set_error("probav_backward: null/invalid argument", hipSuccess); return PROBAV_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const Plan p = make_plan(e, B, 1);
    if (ws_bytes < (scratch ? p.fwd_total : p.total) * sizeof(float)) { set_error("probav_backward: workspace too small", hipSuccess); return PROBAV_ENOSPACE; }
    if (scratch && scratch_bytes < p.bwd_total * sizeof(float)) { set_error("probav_backward: scratch too small", hipSuccess); return PROBAV_ENOSPACE; }
    if (dx && (e->cfg.num_filters != 32 || !input_grad_supported(e->Hin, e->cfg.num_img_lr, e->cfg.in_channels))) {
        set_error("probav_backward_input: the input-gradient kernel needs num_filters == 32 and a tile of all frames inside its LDS budget", hipSuccess);
        return PROBAV_EINVAL;
    }
    CK(device_tables(e));
    const float* W = (const float*)ws;
    float* S = scratch ? (float*)scratch : const_cast<float*>(W) + p.fwd_total;
    const Net& n = p.net;
    const Derived dv = derived(e, p, W, WC);
    const int R = e->cfg.num_res_blocks;
    auto weff = [&](int li) { return dv.weff + e->layers[li].wn.w_off; };
    const PassBufs pb = {e, dv, params, S + p.dweff2, grads, S + p.partial};
    auto filter = [&](Role role, int i = 0) { return launch_at(p, role, LaunchKind::wgrad, true, i); };
    auto data = [&](Role role, int i = 0) { return launch_at(p, role, LaunchKind::conv, true, i); };
    // amax slots of the gradient tensors, in list order (the forward pass left those of the weights and activations): k-th of the arrays the launch's output takes
    const bool h3 = e->fam.arith == 2;
    const AmaxSlots A(e, p, W, dv.wslots, S);
    auto slot_of = [&](const Launch& L, int k = 0) -> unsigned* { return h3 && k < L.slots ? A.back(L.slot + k) : nullptr; };
    auto amx = [&](const unsigned* ax, int li, unsigned* ay) { Amax m; if (h3) { m.x = ax; m.w = A.wrow(li); m.y = ay; } return m; };   // backward-data: the matrix' columns are the layer's INPUT channels
    if (e->fwd_gemm_arith != e->fam.gemm_arith) {
        set_error("probav_backward: the general matrix route's arithmetic changed between forward and backward (probav_engine_set_gemm_x6, or a switch it depends on): the recomputed expConv would not take the forward's gates", hipSuccess);
        return PROBAV_EINVAL;
    }
    if (e->fwd_gemm_exotic != e->fam.gemm_exotic) {
        set_error("probav_backward: the route's exotic launches changed hands between forward and backward (probav_engine_set_gemm_exotic, or a switch it depends on): the reverse scratch was sized for the forward's", hipSuccess);
        return PROBAV_EINVAL;
    }
    if (e->fwd_pair != e->fam.pw_fused) {
        set_error("probav_backward: the pointwise pair's form changed between forward and backward (the kernel family, impl 0 <-> >= 1, or a route switch): the workspace layout differs", hipSuccess);
        return PROBAV_EINVAL;
    }
    if (h3 && !e->fwd_amax) {
        set_error("probav_backward: the H3 kernels (impl 4) need the amax slots of a forward pass run with the same kernel family", hipSuccess);
        return PROBAV_EINVAL;
    }
    // (the reverse pass's per-sample amax slots are cleared by tail_bwd_kernel, its first launch)
    auto dweff = [&](int li) { return S + p.dweff2 + e->layers[li].wn.w_off; };
    auto dbias = [&](int li) { return grads + e->layers[li].wn.b_off; };
    // (defer: the slab sums and the small launches that only the weight-norm backward waits for are queued and leave in a few flushes -- one event record
    // on the launch stream per flush instead of one per launch, probav_common.h)
    SideGuard side_guard((side_stream_disabled() || e->side_mode == 0) ? nullptr : engine_side(e), s, 1);

    CK(tail_backward(dy, S + p.dtail, B, n.up.Ho, e->cfg.scale, e->cfg.std, s, h3 ? A.back(0) : nullptr, h3 ? p.n_amax - p.amax_bwd : 0));
    // low-frequency residual path (models/modelsTF.py:45-53), last layer first: beside the main chain, nothing below depends on it until the weight-norm
    // backward -- queued and launched at the first flush, when the launch stream has its next kernels
    const Launch path = launch_at(p, Role::resid_path, LaunchKind::fused, true);
    {
        // (the queued launch runs later, from reduce_flush: everything it needs is captured BY VALUE -- pointers, launch-list entries and extents, nothing of this frame)
        const float *r2 = W + p.r2, *r1 = W + p.r1, *mn = W + p.mn;
        float *dtail = S + p.dtail, *dr2 = S + p.dr2, *dr1 = S + p.dr1;
        if (path.kind == LaunchKind::fused) {
            if (resid_path_slab_floats(B, path.g.Cin) > path.slab.floats) { set_error("probav_backward: the fused residual path needs a larger slab region than make_plan laid out", hipSuccess); return PROBAV_EINVAL; }
            float *dw3 = dweff(e->iResid3), *db3 = dbias(e->iResid3), *dw2 = dweff(e->iResid2), *db2 = dbias(e->iResid2), *dw1 = dweff(e->iResid1), *db1 = dbias(e->iResid1);
            const float *w2r = weff(e->iResid2), *w3r = weff(e->iResid3);
            float* const slabs = pb.slabs + path.slab.off;
            float* const dr1_out = dx ? dr1 : nullptr;         // the gated gradient at residConv1, which the kernel otherwise keeps in LDS: only the input gradient reads it
            CK(reduce_later(s, [=](hipStream_t rs) -> int {    // one launch + one slab sum (the region holds the patches' slabs: make_plan sized it)
                return resid_path_backward(B, path.g.Hi, path.g.Cin, mn, r1, r2, dtail, w2r, w3r, dw1, db1, dw2, db2, dw3, db3, slabs, rs, dr1_out); }));
        } else {
        const Launch f3 = filter(Role::resid3), d3 = data(Role::resid3), f2 = filter(Role::resid2), d2 = data(Role::resid2), f1 = filter(Role::resid1);
        CK(reduce_later(s, [=](hipStream_t rs) -> int {
            CK(conv_wgrad(pb, f3, r2, dtail, nullptr, Amax(), rs));
            CK(conv_fwd(pb, d3, dtail, nullptr, nullptr, dr2, Amax(), rs));
            CK(conv_wgrad(pb, f2, r1, dr2, nullptr, Amax(), rs));
            CK(conv_fwd(pb, d2, dr2, nullptr, nullptr, dr1, Amax(), rs));
            CK(conv_wgrad(pb, f1, mn, dr1, r1, Amax(), rs));
            return PROBAV_OK;
        }));
        }
    }
    // upscale + reducers (models/modelsTF.py:152-164)
    const int nred = (int)n.red.size();
    float* cur = S + p.gA;
    float* oth = S + p.gB;                          // (the unfused block path below ping-pongs between `cur` and this)
    unsigned* acur;                                 // amax slot of the tensor `cur` holds
    {
        const Launch fu = filter(Role::up), du = data(Role::up);
        const float* const upx = W + p.red[nred - 1];
        float* const updy = S + p.dtail;
        CK(reduce_later(s, [=](hipStream_t rs) -> int {       // (only the weight-norm backward reads it; captured by value: it runs from a later flush)
            return conv_wgrad(pb, fu, upx, updy, nullptr, Amax(), rs); }));
        acur = slot_of(du);
        CK(conv_fwd(pb, du, S + p.dtail, nullptr, nullptr, cur, amx(nullptr, e->iUp, acur), s));
    }
    for (int k = nred - 1; k >= 0; --k) {
        const Launch dr = data(Role::red, k);
        const ConvGeom& gr = n.red[k];
        const float* xin = k ? W + p.red[k - 1] : W + p.act[R];
        // the backward-filter only feeds the weight-norm backward at the very end: side stream; every tensor it reads stays untouched
        // (each stage of the chain writes a buffer of its own)
        { Amax m; if (h3) { m.x = k ? A.red(k - 1) : A.act(R); m.w = acur; }
          CK(conv_wgrad(pb, filter(Role::red, k), xin, cur, W + p.red[k], m, e->side_mode >= 2 ? reduce_fork(s) : s)); }
        float* outA = S + p.gred[2 * k];
        float* outB = S + p.gred[2 * k + 1];
        unsigned* aoth = slot_of(dr);
        CK(conv_fwd(pb, dr, cur, W + p.red[k], nullptr, outA, amx(acur, e->iRed[k], aoth), s));
        if (dr.slots == 2) {                        // mirrored pads: the folded gradient is a new tensor
            acur = slot_of(dr, 1);
            if (gr.ph == 1 && !gr.reflect_t) CK(reflect_fold(outA, outB, B, gr.Hi, gr.Wi, gr.Ti * gr.Cin, acur, s));
            else {
                CK(reflect_fold3(outA, outB, B, gr.Hi, gr.Wi, gr.Ti, gr.Cin, gr.ph, gr.pw, gr.reflect_t ? gr.pt : 0, s));
                if (h3) CK(amax_tensor(outB, in_floats(gr) / B, B, acur, s));
            }
            cur = outB;
        } else {
            cur = outA;
            acur = aoth;
        }
    }
    // residual blocks (models/modelsTF.py:177-189), last first.  cur = d loss / d act[i+1]
    const ConvGeom &ge = n.exp, &gd = n.dec;
    CK(reduce_flush(s));                                   // the residual path, the upscale layer's backward-filter, the reducers' slab sums: one fork
    for (int i = R - 1; i >= 0; --i) {
        float* gDec = S + p.gDec;
        float* Hbuf = S + p.Hb;
        float* dH = S + p.dH;
        // normConv_i: d loss/d w, then d loss/d dec_i
        const Launch pair = launch_at(p, Role::pair, LaunchKind::fused, true, i), dn = data(Role::norm, i);
        const bool fusedp = pair.kind == LaunchKind::fused;
        { Amax m; if (h3) { m.x = A.dec(i); m.w = acur; }
          // (from the second block on, the last thing enqueued on s was the previous block's pointwise backward, whose slab sums forked right behind it)
          CK(conv_wgrad(pb, filter(Role::norm, i), W + p.dec[i], cur, nullptr, m,
                        (fusedp && e->side_mode >= 2) ? (i < R - 1 ? reduce_fork_adjacent(s) : reduce_fork(s)) : s)); }
        if (fusedp) oth = S + p.gblk[i];                   // this block's dX goes to its own buffer: `cur` stays intact for the late backward-filter
        unsigned* agdec = slot_of(dn);
        CK(conv_fwd(pb, dn, cur, nullptr, nullptr, gDec, amx(acur, e->iNorm[i], agdec), s));
        if (fusedp) {
            // fused: H recompute, dH, ReLU gate, dX (+ skip), dW1, dW2, db1, db2 -- nothing 256-wide touches HBM
            unsigned* anew = slot_of(pair);                  // amax slot of dX
            {   // (the class's bracket ends HERE: the flush below launches the batched slab sums on this stream, and they are no part of this class)
            const bool gp = e->fam.pw_fused == PairKind::gemm;
            // bwd-data + bwd-filter of expConv and decConv; the recompute of H (F*E more) is not algorithmic work of the tuned pair.  The general pair books it
            // (3 F H + 2 H D per voxel), as the un-fused route's recomputing launch does
            ProfScope ps(e, (e->fam.x6 && !gp) ? CLS_PW_BWD_DATA_X6 : CLS_PW_BWD_DATA, (gp ? 3.0 : 2.0) * geom_macs(ge) + 2.0 * geom_macs(gd), s);
            if (gp) CK(gemm_pair_backward_launch(pb, pair, W + p.act[i], gDec, cur, oth, anew, s));
            else CK(pw_backward_launch(pb, pair, A, W + p.act[i], gDec, cur, oth, agdec, anew, s));
            }
            float* tmp2 = cur; cur = oth; oth = tmp2;
            acur = anew;
            // what has been queued leaves every fourth block, and before the last one: the small launches to the side stream, the slab sums as ONE kernel on this stream
            // (round 5: slab_sum_later; one flush at the very end instead measured the same, +0.1 %)
            if (((R - 1 - i) & 3) == 3 || i == 1) CK(reduce_flush(s));
            continue;
        }
        // recompute H = relu(expConv_i(act[i])): the 256-channel tensor is never kept (1 KB/voxel/block)
        CK(conv_fwd(pb, data(Role::hidden, i), W + p.act[i], nullptr, nullptr, Hbuf, Amax(), s));
        // decConv_i
        CK(conv_wgrad(pb, filter(Role::dec, i), Hbuf, gDec, nullptr, Amax(), s));
        CK(conv_fwd(pb, data(Role::dec, i), gDec, nullptr, nullptr, dH, Amax(), s));
        // expConv_i: ReLU gate (H > 0) applied where dH is consumed; skip path adds d loss/d act[i+1]
        CK(conv_wgrad(pb, filter(Role::exp, i), W + p.act[i], dH, Hbuf, Amax(), s));
        const Launch de = data(Role::exp, i);
        unsigned* aoth = slot_of(de);
        CK(conv_fwd(pb, de, dH, Hbuf, cur, oth, amx(nullptr, e->iExp[i], aoth), s));
        float* tmp = cur; cur = oth; oth = tmp;
        acur = aoth;
    }
    // mainConv1 (input-facing: no backward-data).  What is still queued leaves first, and this layer's own slab sum stays on the launch stream: forked, the
    // weight-norm backward would wait for an event record, a 10-us kernel on the side stream and the join's record -- 45 us of hole at the end of the pass.
    CK(reduce_flush(s));
    {
        ReduceSide* const ctx = side_guard.c;
        reduce_side_activate(nullptr);
        const int rc = conv_wgrad(pb, filter(Role::main), W + p.xn, cur, W + p.act[0], Amax(), s);
        reduce_side_activate(ctx);
        if (rc) return rc;
    }
    CK(reduce_join(s));                                                       // every slab sum has landed in dweff / the bias gradients
    if (dx) {
        // d loss / d x (models/modelsTF.py:23-27, 45-47, 58 in reverse): mainConv1's backward-data on the gated `cur`, and residConv1's on the residual path's
        // d r1 -- which has arrived with the join -- spread over the frames.  Fused residual path: dr1 holds the gated gradient; un-fused: the plain
        // backward-data output, gated here by r1 as its backward-filter gates it
        CK(input_grad(B, e->Hin, e->cfg.num_img_lr, e->cfg.in_channels, cur, W + p.act[0], weff(e->iMain), S + p.dr1,
                      path.kind == LaunchKind::fused ? nullptr : W + p.r1, weff(e->iResid1), e->cfg.std, dx, s));
    }
    { ProfScope ps(e, CLS_WN, 0.0, s); CK(wn_backward(e->d_layers, (int)e->layers.size(), (int)e->cout_total, params, S + p.dweff2, dv.invn, grads, s)); }
    return PROBAV_OK;
}

int probav_backward(probav_engine* e, const float* params, const float* dy, float* grads, void* ws, size_t ws_bytes, int B, void* stream)
{
    return backward_impl(e, params, dy, grads, ws, ws_bytes, nullptr, 0, B, nullptr, stream);
}
int probav_backward_split(probav_engine* e, const float* params, const float* dy, float* grads, const void* saved, size_t saved_bytes,
                          void* scratch, size_t scratch_bytes, int B, const void* wcache, size_t wcache_bytes, void* stream)
{
    if (!scratch) { set_error("probav_backward_split: null scratch", hipSuccess); return PROBAV_EINVAL; }
    if (wcache && !e) { set_error("probav_backward_split: null engine", hipSuccess); return PROBAV_EINVAL; }
    if (wcache && wcache_bytes < make_wc_plan(e).total * sizeof(float)) { set_error("probav_backward_split: weight cache too small", hipSuccess); return PROBAV_ENOSPACE; }
    return backward_impl(e, params, dy, grads, saved, saved_bytes, scratch, scratch_bytes, B, (const float*)wcache, stream);
}
int probav_backward_input(probav_engine* e, const float* params, const float* dy, float* grads, const void* saved, size_t saved_bytes,
                          void* scratch, size_t scratch_bytes, int B, const void* wcache, size_t wcache_bytes, float* dx, void* stream)
{
    if (!scratch || !dx) { set_error("probav_backward_input: null scratch / dx", hipSuccess); return PROBAV_EINVAL; }
    if (wcache && !e) { set_error("probav_backward_input: null engine", hipSuccess); return PROBAV_EINVAL; }
    if (wcache && wcache_bytes < make_wc_plan(e).total * sizeof(float)) { set_error("probav_backward_input: weight cache too small", hipSuccess); return PROBAV_ENOSPACE; }
    return backward_impl(e, params, dy, grads, saved, saved_bytes, scratch, scratch_bytes, B, (const float*)wcache, stream, dx);
}
int probav_input_grad(int batch, int H, int T, int C, const float* g, const float* act0, const float* wmain, const float* d1,
                      const float* gate1, const float* w1, float stdv, float* dx, void* stream)
{
    return input_grad(batch, H, T, C, g, act0, wmain, d1, gate1, w1, stdv, dx, (hipStream_t)stream);
}
int probav_workspace_split(const probav_engine* e, int batch, size_t* saved_bytes, size_t* scratch_bytes)
{
    if (!e || batch < 1 || !saved_bytes || !scratch_bytes) { set_error("probav_workspace_split: null/invalid argument", hipSuccess); return PROBAV_EINVAL; }
    const Plan p = make_plan(e, batch, 1);
    *saved_bytes = p.fwd_total * sizeof(float);
    *scratch_bytes = p.bwd_total * sizeof(float);
    return PROBAV_OK;
}
int probav_backward_wc(probav_engine* e, const float* params, const float* dy, float* grads, void* ws, size_t ws_bytes, int B,
                       const void* wcache, size_t wcache_bytes, void* stream)
{
    if (!e || !wcache) { set_error("probav_backward_wc: null engine / weight cache", hipSuccess); return PROBAV_EINVAL; }
    if (wcache_bytes < make_wc_plan(e).total * sizeof(float)) { set_error("probav_backward_wc: weight cache too small", hipSuccess); return PROBAV_ENOSPACE; }
    return backward_impl(e, params, dy, grads, ws, ws_bytes, nullptr, 0, B, (const float*)wcache, stream);
}

size_t probav_weight_cache_bytes(const probav_engine* e) { return e ? make_wc_plan(e).total * sizeof(float) : 0; }

// The one writer of a weight cache: checks, layout, device tables, amax reset, the launch `fill(wc, C, wam, s)` that writes the effective weights, inverse
// norms and amax slots into the cache C, and the operand packing behind it.  `who`: the entry point's name, for its error messages
static int write_weight_cache(probav_engine* e, const char* who, bool args_ok, void* wcache, size_t wcache_bytes, void* stream,
                              const std::function<int(const WcPlan&, float*, unsigned*, hipStream_t)>& fill)
{
    const std::string name(who);
    if (!args_ok) { set_error((name + ": null argument").c_str(), hipSuccess); return PROBAV_EINVAL; }
    const WcPlan wc = make_wc_plan(e);
    if (wcache_bytes < wc.total * sizeof(float)) { set_error((name + ": weight cache too small").c_str(), hipSuccess); return PROBAV_ENOSPACE; }
    CK(device_tables(e));
    hipStream_t s = (hipStream_t)stream;
    float* C = (float*)wcache;
    unsigned* wam = reinterpret_cast<unsigned*>(C + wc.amax);
    if (hipMemsetAsync(wam, 0, (size_t)wc.n_wamax * sizeof(unsigned), s) != hipSuccess) { set_error((name + ": amax reset").c_str(), hipGetLastError()); return PROBAV_EHIP; }
    { ProfScope ps(e, CLS_WN, 0.0, s); CK(fill(wc, C, wam, s)); }
    if (!e->jobs.empty()) { ProfScope ps(e, CLS_WN, 0.0, s); CK(mfma_pack(e->d_jobs, (int)e->jobs.size(), C + wc.weff, C + wc.weffT, C + wc.wpack, wam, s)); }
    return PROBAV_OK;
}

int probav_optimizer_step_fused(probav_engine* e, float* params, const float* grads, float* m, float* v, float lr, float beta1, float beta2,
                                float eps, float c_g, float c_m, float c_v, void* wcache, size_t wcache_bytes, void* stream)
{
    // one launch: the update of all 132 tensors + the weight normalisation of the updated parameters (+ the per-row maxima and the operand
    // packing of the next pass behind it): the next probav_forward_wc starts at the head kernel
    return write_weight_cache(e, "probav_optimizer_step_fused", e && params && grads && m && v && wcache, wcache, wcache_bytes, stream,
        [&](const WcPlan& wc, float* C, unsigned* wam, hipStream_t s) {
            return optimizer_wn_step(e->d_layers, (int)e->layers.size(), (int)e->cout_total, (int)e->cin_total, params, grads, m, v, lr, beta1, beta2, eps, c_g, c_m, c_v,
                                     C + wc.weff, C + wc.weffT, C + wc.invn, wam, s); });
}

int probav_optimizer_step_fused_guarded(probav_engine* e, float* params, const float* grads, float* m, float* v, float lr, float beta1, float beta2,
                                        float eps, float c_g, float c_m, float c_v, void* wcache, size_t wcache_bytes, float* ema, float ema_momentum,
                                        const probav_guard_ctl* ctl, void* stream)
{
    const bool args_ok = e && params && grads && m && v && wcache;
    if (args_ok && ema && !(ema_momentum >= 0.f && ema_momentum <= 1.f)) { set_error("probav_optimizer_step_fused_guarded: ema_momentum outside [0, 1]", hipSuccess); return PROBAV_EINVAL; }
    // probav_optimizer_step_fused with the control block and the EMA buffer handed to the update half; on a skipped step the same launches rebuild the
    // cache of the unchanged parameters
    return write_weight_cache(e, "probav_optimizer_step_fused_guarded", args_ok, wcache, wcache_bytes, stream,
        [&](const WcPlan& wc, float* C, unsigned* wam, hipStream_t s) {
            return optimizer_wn_step_guarded(e->d_layers, (int)e->layers.size(), (int)e->cout_total, (int)e->cin_total, params, grads, m, v, lr, beta1, beta2, eps, c_g, c_m, c_v,
                                             C + wc.weff, C + wc.weffT, C + wc.invn, wam, ema, ema_momentum, ctl, s); });
}

int probav_weight_cache_build(probav_engine* e, const float* params, void* wcache, size_t wcache_bytes, void* stream)
{
    // exactly what a forward pass without a cache does first: weight normalisation (+ per-column / per-row maxima) and operand packing
    return write_weight_cache(e, "probav_weight_cache_build", e && params && wcache, wcache, wcache_bytes, stream,
        [&](const WcPlan& wc, float* C, unsigned* wam, hipStream_t s) {
            return wn_forward(e->d_layers, (int)e->layers.size(), (int)e->cout_total, (int)e->cin_total, params, C + wc.weff, C + wc.weffT, C + wc.invn, wam, s); });
}

// ---- introspection (parity tests) -----------------------------------------------------------------
int probav_workspace_view(const probav_engine* e, int batch, int training, int kind, int index, int64_t* offset_floats, int64_t* count)
{
    if (!e || batch < 1 || !offset_floats || !count) { set_error("probav_workspace_view: null/invalid argument", hipSuccess); return PROBAV_EINVAL; }
    const Plan p = make_plan(e, batch, training);
    const Net& n = p.net;
    const int R = e->cfg.num_res_blocks, nred = (int)n.red.size();
    switch (kind) {
    case PROBAV_VIEW_ACT: if (index < 0 || index > R) break; *offset_floats = (int64_t)p.act[index]; *count = (int64_t)out_floats(n.main); return PROBAV_OK;
    case PROBAV_VIEW_DEC: if (index < 0 || index >= R) break; *offset_floats = (int64_t)p.dec[index]; *count = (int64_t)out_floats(n.dec); return PROBAV_OK;
    case PROBAV_VIEW_RED: if (index < 0 || index >= nred) break; *offset_floats = (int64_t)p.red[index]; *count = (int64_t)out_floats(n.red[index]); return PROBAV_OK;
    case PROBAV_VIEW_RESID1: if (index != 0) break; *offset_floats = (int64_t)p.r1; *count = (int64_t)out_floats(n.resid1); return PROBAV_OK;
    case PROBAV_VIEW_INPUT: if (index != 0) break; *offset_floats = (int64_t)p.xn; *count = (int64_t)in_floats(n.main); return PROBAV_OK;
    default: break;
    }
    set_error("probav_workspace_view: no such tensor", hipSuccess);
    return PROBAV_EINVAL;
}

int probav_debug_hidden(probav_engine* e, const float* params, const void* ws, size_t ws_bytes, int B, int block, float* hidden, float* dec_scratch, const void* wcache, void* stream)
{
    if (!e || !params || !ws || !hidden || !dec_scratch || B < 1 || block < 0 || block >= e->cfg.num_res_blocks) { set_error("probav_debug_hidden: null/invalid argument", hipSuccess); return PROBAV_EINVAL; }
    if (e->fam.pw_fused == PairKind::gemm) {
        // the general fused pair, in every family that has it: its forward launch again with the dump pointer, into the caller's scratch; the saved state is only read
        const Plan p = make_plan(e, B, 1);
        if (ws_bytes < p.fwd_total * sizeof(float)) { set_error("probav_debug_hidden: workspace too small", hipSuccess); return PROBAV_ENOSPACE; }
        const float* W = (const float*)ws;
        return gemm_pair_forward_launch(e, block, derived(e, p, W, (const float*)wcache), params, W + p.act[block], dec_scratch, p.net.exp, nullptr, (hipStream_t)stream, hidden);
    }
    if (e->fam.pw_fused == PairKind::none && e->fam.gemm_arith == 1) {
        // the un-fused route in x6 arithmetic: the launch the reverse pass recomputes the hidden tensor with (Role::hidden), which is the forward's expConv launch
        // again -- the gates the gradient was taken at.  (In fp32 arithmetic the route's bits are the direct kernel's, and probav_conv3d_forward gives them.)
        const Plan p = make_plan(e, B, 1);
        if (ws_bytes < p.fwd_total * sizeof(float)) { set_error("probav_debug_hidden: workspace too small", hipSuccess); return PROBAV_ENOSPACE; }
        const Launch L = launch_at(p, Role::hidden, LaunchKind::conv, true, block);
        const ConvRoute r = conv_route(e->fam, L.g, L.o);
        if (L.kind != LaunchKind::conv || r.k != ConvKernel::gemm || r.arith != 1) { set_error("probav_debug_hidden: the recomputed expConv is not a launch of the x6 route", hipSuccess); return PROBAV_EINVAL; }
        const float* W = (const float*)ws;
        const Derived dv = derived(e, p, W, (const float*)wcache);
        const WnLayer& wn = e->layers[e->iExp[block]].wn;
        return gemm_x6_conv_forward(L.g, W + p.act[block], nullptr, dv.weff + wn.w_off, params + wn.b_off, nullptr, hidden, (hipStream_t)stream);
    }
    if (!e->fam.x6 || e->fam.pw_fused != PairKind::tuned) { set_error("probav_debug_hidden: only the split-operand kernel families (impl 3, 4) expose their hidden tile", hipSuccess); return PROBAV_EINVAL; }
    const Plan p = make_plan(e, B, 1);
    if (ws_bytes < p.fwd_total * sizeof(float)) { set_error("probav_debug_hidden: workspace too small", hipSuccess); return PROBAV_ENOSPACE; }
    const float* W = (const float*)ws;
    const Derived dv = derived(e, p, W, (const float*)wcache);        // (the forward pass ran from the weight cache: its fragments and weight slots live there)
    const AmaxSlots A(e, p, W, dv.wslots);
    // the forward launch of block i again, into the caller's scratch output (the saved state is only read), with the hidden tile written out;
    // no amax report (the slots of the saved tensors stay as the forward pass left them)
    return pw_forward_launch(e, block, dv.wpack, A, params, W + p.act[block], dec_scratch, in_voxels(p.net.exp), nullptr, (hipStream_t)stream, hidden);
}

int probav_debug_hidden_from_forward_kernel(int on) { x6_pw_dump_from_forward_kernel(on); return PROBAV_OK; }

// ---- single operators ---------------------------------------------------------------------------
static ConvGeom geom_from(const int32_t a[17])
{
    ConvGeom g;
    g.N = a[0]; g.Hi = a[1]; g.Wi = a[2]; g.Ti = a[3]; g.Cin = a[4]; g.Ho = a[5]; g.Wo = a[6]; g.To = a[7]; g.Cout = a[8];
    g.kh = a[9]; g.kw = a[10]; g.kt = a[11]; g.ph = a[12]; g.pw = a[13]; g.pt = a[14]; g.reflect_hw = a[15]; g.relu = a[16]; g.reflect_t = 0;
    return g;
}
static bool geom_ok(const ConvGeom& g)
{
    if (g.N < 1 || g.Cin < 1 || g.Cout < 1 || g.kh < 1 || g.kw < 1 || g.kt < 1) return false;
    if (g.Ho < 1 || g.Wo < 1 || g.To < 1 || g.Hi < 1 || g.Wi < 1 || g.Ti < 1) return false;
    if (g.ph < 0 || g.pw < 0 || g.pt < 0) return false;
    if (g.reflect_hw && (g.ph >= g.Hi || g.pw >= g.Wi || g.kh - 1 - g.ph >= g.Hi || g.kw - 1 - g.pw >= g.Wi)) return false;
    return true;
}

// Scratch owned by the library for the single-operator entry points (parity tests), allocated on first use -- the engine path never does this.
// Packing raw Keras-layout weights into MFMA fragments needs a device buffer (a conv area, then the pointwise pair's four fragments) and a job
// table; an H3 call needs amax slots (the engine gets them from the producing kernels).
constexpr size_t OP_CONV_FLOATS = (size_t)1 << 20, OP_PW_FLOATS = 4 * X6_PW_FRAG_WORDS;     // (X6: the largest pointwise fragments)
static struct { float* frag; PackJob* jobs; unsigned* amax; size_t amax_cap; } g_op;
static int op_scratch()
{
    hipError_t err = hipSuccess;
    if (!g_op.frag) err = hipMalloc((void**)&g_op.frag, (OP_CONV_FLOATS + OP_PW_FLOATS) * sizeof(float));
    if (err == hipSuccess && !g_op.jobs) err = hipMalloc((void**)&g_op.jobs, 4 * sizeof(PackJob));
    if (err != hipSuccess) { set_error("single-operator scratch allocation", err); return PROBAV_EHIP; }
    return PROBAV_OK;
}
// `count` zeroed slots in g_op.amax
static int op_amax_reserve(size_t count, hipStream_t s)
{
    if (count > g_op.amax_cap) {
        hipError_t err = hipStreamSynchronize(s);
        if (err == hipSuccess && g_op.amax) err = hipFree(g_op.amax);
        g_op.amax = nullptr; g_op.amax_cap = 0;
        if (err == hipSuccess) err = hipMalloc((void**)&g_op.amax, (count + 1024) * sizeof(unsigned));
        if (err != hipSuccess) { set_error("single-operator amax allocation", err); return PROBAV_EHIP; }
        g_op.amax_cap = count + 1024;
    }
    if (hipMemsetAsync(g_op.amax, 0, count * sizeof(unsigned), s) != hipSuccess) { set_error("single-operator amax reset", hipGetLastError()); return PROBAV_EHIP; }
    return PROBAV_OK;
}
// convolution operands: slots [0, N) = x per sample, [N, 2N) = output / dY per sample, [2N, 2N + cols) = filter per output column
static int op_amax_conv(const ConvGeom& g, const float* x, const float* w, const float* dy, hipStream_t s)
{
    int rc = op_amax_reserve((size_t)2 * g.N + 256, s);
    if (!rc) rc = amax_tensor(x, (size_t)g.Hi * g.Wi * g.Ti * g.Cin, g.N, g_op.amax, s);
    if (!rc && dy) rc = amax_tensor(dy, (size_t)g.Ho * g.Wo * g.To * g.Cout, g.N, g_op.amax + g.N, s);
    if (!rc && w) rc = amax_columns(w, (long)g.kh * g.kw * g.kt * g.Cin, g.Cout, g_op.amax + 2 * g.N, s);
    return rc;
}
// packs `n` jobs into g_op.frag once the stream has drained (the previous call may still read the fragments)
static int op_pack_jobs(const PackJob* J, int n, const float* weff, const float* weffT, hipStream_t s, const char* what)
{
    hipError_t err = hipStreamSynchronize(s);
    if (err == hipSuccess) err = hipMemcpy(g_op.jobs, J, n * sizeof(PackJob), hipMemcpyHostToDevice);
    if (err != hipSuccess) { set_error(what, err); return PROBAV_EHIP; }
    return mfma_pack(g_op.jobs, n, weff, weffT, g_op.frag, g_op.amax, s);
}
// the filter of a convolution in arithmetic `arith` (per_tap: the per-tap H3 form of 25 channels) -> g_op.frag
static int op_pack(const ConvGeom& g, const float* w, hipStream_t s, int arith, bool per_tap)
{
    PackJob J = pack_job(per_tap ? Operand::conv_taps : Operand::conv, arith, g.Cin, g.Cout);
    if (J.count == 0) { set_error("probav_conv3d_forward: channel configuration not supported by the MFMA kernel", hipSuccess); return PROBAV_EINVAL; }
    CK(op_scratch());
    if ((size_t)J.count > OP_CONV_FLOATS) { set_error("probav_conv3d_forward: fragment scratch too small", hipSuccess); return PROBAV_ENOSPACE; }
    if (arith == 2) J.amax_slot = 2 * g.N;
    return op_pack_jobs(&J, 1, w, w, s, "probav_conv3d_forward: job upload");
}

// The kernel that serves a single-operator convolution call: the one decision probav_conv3d_forward (launch) and probav_plan_conv (report) read.  Only WHICH of gate / bias /
// skip exist matters.  impl 0 the direct kernel; impl 1 the MFMA row-tile kernel, 2 the strip kernel, 3 / 4 the x6 strip kernel (X6 / H3; the piece-ring form where it applies) or,
// where the strip kernels do not apply, its row-tile form: what conv_route gives family `impl` behind the engine's dedicated kernels, anything else is refused
enum class OpConvKernel { up, up_bwd_data, direct, routed, refused };
// the operands of a single-operator call as the routes see them: every kind of filter fragment (the caller packs what the route chooses), and under impl 4 the inputs' amax
static Operands op_operands(bool gate, bool bias, bool skip, int impl)
{
    Operands o;
    o.gate = gate; o.bias = bias; o.skip = skip; o.f32 = o.x6 = o.h3 = o.h3t = true; o.am_in = impl == 4;
    return o;
}
struct OpConvRoute { OpConvKernel k; ConvRoute r; };
static OpConvRoute op_conv_route(const ConvGeom& g, bool gate, bool bias, bool skip, int impl)
{
    // (what the engine does for these two geometries in every kernel family but 0)
    if (impl >= 1 && !gate && !skip && bias && conv3d_up_forward_supported(g)) return {OpConvKernel::up, {}};
    if (impl >= 1 && !gate && !skip && !g.relu && conv3d_up_bwd_data_supported(g)) return {OpConvKernel::up_bwd_data, {}};
    if (impl == 0) return {OpConvKernel::direct, {}};
    const ConvRoute r = conv_route(make_family(impl, false), g, op_operands(gate, bias, skip, impl), false);
    const bool documented = impl == 1 ? r.k == ConvKernel::mfma_rowtile : (impl == 2 ? r.k == ConvKernel::mfma_strip : r.k == ConvKernel::x6_strip || r.k == ConvKernel::x6_rowtile);
    return {documented ? OpConvKernel::routed : OpConvKernel::refused, r};
}

int probav_conv3d_forward(const int32_t geom[17], const float* x, const float* gate, const float* w, const float* bias,
                          const float* skip, float* y, int impl, void* stream)
{
    if (!geom || !x || !w || !y) { set_error("probav_conv3d_forward: null argument", hipSuccess); return PROBAV_EINVAL; }
    const ConvGeom g = geom_from(geom);
    if (!geom_ok(g)) { set_error("probav_conv3d_forward: bad geometry", hipSuccess); return PROBAV_EINVAL; }
    if (impl < 0 || impl > 4) { set_error("probav_conv3d_forward: impl must be 0..4", hipSuccess); return PROBAV_EINVAL; }
    const hipStream_t s = (hipStream_t)stream;
    const OpConvRoute o = op_conv_route(g, gate != nullptr, bias != nullptr, skip != nullptr, impl);
    if (o.k == OpConvKernel::up) return conv3d_up_forward(g, x, w, bias, y, s);
    if (o.k == OpConvKernel::up_bwd_data) return conv3d_up_bwd_data(g, x, w, bias, y, nullptr, s);
    if (o.k == OpConvKernel::direct) return conv3d_direct_forward(g, x, gate, w, bias, skip, y, s);
    if (o.k == OpConvKernel::refused) { set_error("probav_conv3d_forward: geometry not supported by this MFMA kernel", hipSuccess); return PROBAV_EINVAL; }
    const ConvRoute& r = o.r;
    Amax am;
    CK(op_scratch());
    if (impl == 4) {
        if (g.Cout > 256) { set_error("probav_conv3d_forward: Cout > 256", hipSuccess); return PROBAV_EINVAL; }
        CK(op_amax_conv(g, x, w, nullptr, s));
        am.x = g_op.amax; am.w = g_op.amax + 2 * g.N; am.y = g_op.amax + g.N;
    }
    CK(op_pack(g, w, s, r.arith, r.strip.taps));
    return conv_launch(r, g, x, gate, w, g_op.frag, bias, skip, y, am, s);
}

// The kernel family that serves a single-operator backward-filter call (impl names a kernel here, not an engine family: 2 is the direct kernel, so the call does not go
// through wgrad_route): read by probav_conv3d_wgrad_scratch_bytes, probav_conv3d_wgrad and probav_plan_conv
enum class OpWgradKernel { x6, mfma, direct, refused };
static OpWgradKernel op_wgrad_kernel(const ConvGeom& g, int impl)
{
    if (impl == 3 || impl == 4) return x6_wgrad_supported(g) ? OpWgradKernel::x6 : OpWgradKernel::refused;
    if (impl == 1) return mfma_wgrad_supported(g) ? OpWgradKernel::mfma : OpWgradKernel::refused;
    return OpWgradKernel::direct;
}

size_t probav_conv3d_wgrad_scratch_bytes(const int32_t geom[17], int impl)
{
    if (!geom) return 0;
    const ConvGeom g = geom_from(geom);
    switch (op_wgrad_kernel(g, impl)) {
    case OpWgradKernel::x6: return x6_wgrad_partial_floats(g) * sizeof(float);
    case OpWgradKernel::mfma: return mfma_wgrad_partial_floats(g) * sizeof(float);
    case OpWgradKernel::direct: return wgrad_partial_floats(g) * sizeof(float);
    default: return 0;
    }
}

int probav_conv3d_wgrad(const int32_t geom[17], const float* x, const float* dy, const float* gate, float* dw, float* db,
                        void* scratch, size_t scratch_bytes, int impl, void* stream)
{
    if (!geom || !x || !dy || !dw || !scratch) { set_error("probav_conv3d_wgrad: null argument", hipSuccess); return PROBAV_EINVAL; }
    const ConvGeom g = geom_from(geom);
    if (!geom_ok(g)) { set_error("probav_conv3d_wgrad: bad geometry", hipSuccess); return PROBAV_EINVAL; }
    const OpWgradKernel k = op_wgrad_kernel(g, impl);
    if (impl == 3 || impl == 4) {
        if (k != OpWgradKernel::x6) { set_error("probav_conv3d_wgrad: geometry not supported by the x6 kernel", hipSuccess); return PROBAV_EINVAL; }
        if (scratch_bytes < x6_wgrad_partial_floats(g) * sizeof(float)) { set_error("probav_conv3d_wgrad: scratch too small", hipSuccess); return PROBAV_ENOSPACE; }
        Amax am;
        if (impl == 4) {
            CK(op_scratch());
            CK(op_amax_conv(g, x, nullptr, dy, (hipStream_t)stream));
            am.x = g_op.amax; am.w = g_op.amax + g.N;
        }
        return x6_conv_wgrad(g, x, dy, gate, dw, db, (float*)scratch, impl == 4 ? 2 : 1, am, (hipStream_t)stream);
    }
    if (impl == 1) {
        if (k != OpWgradKernel::mfma) { set_error("probav_conv3d_wgrad: geometry not supported by the MFMA kernel", hipSuccess); return PROBAV_EINVAL; }
        if (scratch_bytes < mfma_wgrad_partial_floats(g) * sizeof(float)) { set_error("probav_conv3d_wgrad: scratch too small", hipSuccess); return PROBAV_ENOSPACE; }
        return mfma_conv_wgrad(g, x, dy, gate, dw, db, (float*)scratch, (hipStream_t)stream);
    }
    if (scratch_bytes < wgrad_partial_floats(g) * sizeof(float)) { set_error("probav_conv3d_wgrad: scratch too small", hipSuccess); return PROBAV_ENOSPACE; }
    return conv3d_direct_wgrad(g, x, dy, gate, dw, db, (float*)scratch, (hipStream_t)stream);
}

// the fused pointwise pair, single-operator form: its four fragments of W1 [32][256], W2 [256][D] in arithmetic `arith`, behind the conv area
// of g_op.frag.  H3: the weights' amax must already be in the slots op_amax_pw lays out (wbase = index of the first weight slot)
static int op_pack_pw(const float* w1, const float* w2, int D, int arith, int wbase, hipStream_t s, PwOps& f)
{
    CK(op_scratch());
    const Operand ops[4] = {Operand::pw_w1, Operand::pw_w2, Operand::pw_w2b, Operand::pw_w1c};
    const int slot[4] = {wbase + 0, wbase + 8, wbase + 1, wbase + 40};
    const float* out[4];
    PackJob J[4];
    for (int k = 0; k < 4; ++k) {
        const bool from_w1 = ops[k] == Operand::pw_w1 || ops[k] == Operand::pw_w1c;
        J[k] = pack_job(ops[k], arith, from_w1 ? 32 : 256, from_w1 ? 256 : D);
        J[k].src_is_T = from_w1 ? 0 : 1;                                                 // weff := w1, weffT := w2
        J[k].dst_off = (long)(OP_CONV_FLOATS + k * X6_PW_FRAG_WORDS);
        if (arith == 2) J[k].amax_slot = slot[k];
        out[k] = g_op.frag + J[k].dst_off;
    }
    f = {out[0], out[1], out[2], out[3]};
    return op_pack_jobs(J, 4, w1, w2, s, "probav_pw: job upload");
}
// amax of the operands of a single-operator call of the fused pointwise pair, ns samples: [0, ns) x, [ns, 2ns) d_dec, [2ns, 3ns) output;
// wbase = 3 ns: +0 w1, +1 w2, +2 b1 (whole tensors), +8 .. w2 per output column, +40 .. w1 per input row
static int op_amax_pw(const float* x, const float* w1, const float* w2, const float* b1, const float* d_dec, long nvox, long vps, int D, hipStream_t s, PwAmax& m)
{
    int rc = op_scratch();
    if (rc) return rc;
    const int ns = (int)(nvox / vps), wb = 3 * ns;
    rc = op_amax_reserve((size_t)wb + 80, s);
    unsigned* a = g_op.amax;
    if (!rc) rc = amax_tensor(x, (size_t)vps * 32, ns, a, s);
    if (!rc && d_dec) rc = amax_tensor(d_dec, (size_t)vps * D, ns, a + ns, s);
    if (!rc) rc = amax_tensor(w1, 32 * 256, 1, a + wb + 0, s);
    if (!rc) rc = amax_tensor(w2, (size_t)256 * D, 1, a + wb + 1, s);
    if (!rc) rc = amax_tensor(b1, 256, 1, a + wb + 2, s);
    if (!rc) rc = amax_columns(w2, 256, D, a + wb + 8, s);
    if (!rc) rc = amax_tensor(w1, 256, 32, a + wb + 40, s);              // rows of W1 [32][256]
    m.x = a; m.dt = a + ns; m.y = a + 2 * ns;
    m.w1 = a + wb; m.w2 = a + wb + 1; m.b1 = a + wb + 2; m.w2c = a + wb + 8; m.w1r = a + wb + 40;
    return rc;
}

// impl 2: the fp32-MFMA kernels, 3 / 4: the split-operand ones (X6 / H3)
int probav_pw_forward(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* dec,
                      int64_t nvox, int64_t vox_per_sample, int D, int impl, void* stream)
{
    if (!x || !w1 || !b1 || !w2 || !b2 || !dec || nvox < 1 || impl < 2 || impl > 4) { set_error("probav_pw_forward: null/invalid argument", hipSuccess); return PROBAV_EINVAL; }
    if (!mfma_pw_supported(32, 256, D)) { set_error("probav_pw_forward: needs F=32, E=256, D<=26", hipSuccess); return PROBAV_EINVAL; }
    long vps = vox_per_sample > 0 ? (long)vox_per_sample : (long)nvox;
    if (nvox % vps) { set_error("probav_pw_forward: nvox is not a multiple of vox_per_sample", hipSuccess); return PROBAV_EINVAL; }
    const hipStream_t s = (hipStream_t)stream;
    PwAmax am;
    if (impl == 4) CK(op_amax_pw(x, w1, w2, b1, nullptr, (long)nvox, vps, D, s, am));
    PwOps f;
    CK(op_pack_pw(w1, w2, D, impl - 2, 3 * (int)(nvox / vps), s, f));
    return pw_forward(impl - 2, f, x, b1, b2, dec, (long)nvox, vps, D, am, s);
}

size_t probav_pw_backward_scratch_bytes(int D) { return mfma_pw_backward_slab_floats(D) * sizeof(float); }

int probav_pw_backward(const float* x, const float* d_dec, const float* d_skip, const float* w1, const float* b1, const float* w2,
                       float* dx, float* dw1, float* db1, float* dw2, float* db2, void* scratch, size_t scratch_bytes,
                       int64_t nvox, int64_t vox_per_sample, int D, int impl, void* stream)
{
    if (!x || !d_dec || !d_skip || !w1 || !b1 || !w2 || !dx || !dw1 || !db1 || !dw2 || !db2 || !scratch || nvox < 1 || impl < 2 || impl > 4) {
        set_error("probav_pw_backward: null/invalid argument", hipSuccess); return PROBAV_EINVAL;
    }
    if (!mfma_pw_supported(32, 256, D)) { set_error("probav_pw_backward: needs F=32, E=256, D<=26", hipSuccess); return PROBAV_EINVAL; }
    if (scratch_bytes < probav_pw_backward_scratch_bytes(D)) { set_error("probav_pw_backward: scratch too small", hipSuccess); return PROBAV_ENOSPACE; }
    long vps = vox_per_sample > 0 ? (long)vox_per_sample : (long)nvox;
    if (nvox % vps) { set_error("probav_pw_backward: nvox is not a multiple of vox_per_sample", hipSuccess); return PROBAV_EINVAL; }
    const hipStream_t s = (hipStream_t)stream;
    PwAmax am;
    if (impl == 4) CK(op_amax_pw(x, w1, w2, b1, d_dec, (long)nvox, vps, D, s, am));
    PwOps f;
    CK(op_pack_pw(w1, w2, D, impl - 2, 3 * (int)(nvox / vps), s, f));
    return pw_backward(impl - 2, f, x, d_dec, d_skip, b1, dx, dw1, dw2, db1, db2, (float*)scratch, (long)nvox, vps, D, am, s);
}

// ---- plan report (host only: nothing is launched, no device is touched) ----
int probav_plan_conv(const int32_t geom[17], int impl, int gated, int has_skip, int op, int32_t report[8])
{
    if (!geom || !report || impl < 0 || impl > 4 || op < PROBAV_PLAN_OP_FORWARD || op > PROBAV_PLAN_OP_WGRAD) { set_error("probav_plan_conv: null/invalid argument", hipSuccess); return PROBAV_EINVAL; }
    const ConvGeom g = geom_from(geom);
    if (!geom_ok(g)) { set_error("probav_plan_conv: bad geometry", hipSuccess); return PROBAV_EINVAL; }
    for (int i = 0; i < 8; ++i) report[i] = 0;
    int32_t &kernel = report[0], &nsplit = report[1], &nstrips = report[2], &SR = report[3], &nslot = report[4], &grid = report[5], &rvp = report[6];
    if (op == PROBAV_PLAN_OP_WGRAD) {
        int v[4] = {0, 0, 0, 0};
        switch (op_wgrad_kernel(g, impl)) {
        case OpWgradKernel::x6: {
            static const int32_t names[4] = {PROBAV_PLAN_NONE, PROBAV_PLAN_WG4, PROBAV_PLAN_WGRAD_X6_H3, PROBAV_PLAN_WGRAD_X6};
            kernel = names[x6_wgrad_plan_ints(g, gated != 0, impl == 4 ? 2 : 1, v)];
            nsplit = v[0]; nstrips = v[1]; SR = v[2]; grid = v[3];
            break;
        }
        case OpWgradKernel::mfma: if (mfma_conv_plan_ints(g, true, v)) { kernel = PROBAV_PLAN_WGRAD_MFMA; SR = v[0]; nstrips = v[1]; grid = v[2]; nsplit = 1; } break;
        case OpWgradKernel::direct: kernel = PROBAV_PLAN_DIRECT; break;
        default: break;
        }
        return PROBAV_OK;
    }
    const OpConvRoute o = op_conv_route(g, gated != 0, op == PROBAV_PLAN_OP_FORWARD, has_skip != 0, impl);
    if (o.k == OpConvKernel::refused) return PROBAV_OK;
    if (o.k != OpConvKernel::routed) { kernel = PROBAV_PLAN_DIRECT; return PROBAV_OK; }      // the VALU kernels: generic, or the two dedicated upscale ones
    if (o.r.k == ConvKernel::x6_rowtile || o.r.k == ConvKernel::mfma_rowtile) {
        int v[3];
        if (mfma_conv_plan_ints(g, false, v)) { kernel = PROBAV_PLAN_ROWTILE; SR = v[0]; nstrips = v[1]; grid = v[2]; nsplit = 1; }
        return PROBAV_OK;
    }
    const StripSel& sel = o.r.strip;
    if (sel.k == StripKernel::cw4) {
        int v[5];
        if (cw4_conv_plan_ints(g, gated != 0, v)) { kernel = PROBAV_PLAN_CW4; nsplit = v[0]; nstrips = v[1]; SR = v[2]; nslot = v[3]; grid = v[4]; }
        return PROBAV_OK;
    }
    kernel = sel.k == StripKernel::pp ? PROBAV_PLAN_PP : (sel.k == StripKernel::pstrip ? PROBAV_PLAN_PSTRIP : PROBAV_PLAN_STRIP);
    nsplit = sel.plan.a.nsplit; nstrips = sel.plan.a.nstrips; SR = sel.plan.a.SR; grid = sel.plan.grid;
    if (sel.k == StripKernel::pp) { nslot = sel.plan.a.nslot; rvp = sel.rvp; }
    return PROBAV_OK;
}

// ---- the general matrix route (kernels_gemm.hip): single operators, plan report, launch census ----
int probav_gemm_conv3d_forward(const int32_t geom[17], const float* x, const float* gate, const float* w, const float* bias,
                               const float* skip, float* y, void* stream)
{
    if (!geom || !x || !w || !y) { set_error("probav_gemm_conv3d_forward: null argument", hipSuccess); return PROBAV_EINVAL; }
    const ConvGeom g = geom_from(geom);
    if (!geom_ok(g)) { set_error("probav_gemm_conv3d_forward: bad geometry", hipSuccess); return PROBAV_EINVAL; }
    if (!gemm_conv_supported(g)) { set_error("probav_gemm_conv3d_forward: geometry not supported by the general matrix route", hipSuccess); return PROBAV_EINVAL; }
    return gemm_conv_forward(g, x, gate, w, bias, skip, y, (hipStream_t)stream);
}

size_t probav_gemm_conv3d_wgrad_scratch_bytes(const int32_t geom[17])
{
    if (!geom) return 0;
    const ConvGeom g = geom_from(geom);
    if (!geom_ok(g) || !gemm_wgrad_supported(g)) return 0;
    return gemm_wgrad_partial_floats(g) * sizeof(float);
}

int probav_gemm_conv3d_wgrad(const int32_t geom[17], const float* x, const float* dy, const float* gate, float* dw, float* db,
                             void* scratch, size_t scratch_bytes, void* stream)
{
    if (!geom || !x || !dy || !dw || !scratch) { set_error("probav_gemm_conv3d_wgrad: null argument", hipSuccess); return PROBAV_EINVAL; }
    const ConvGeom g = geom_from(geom);
    if (!geom_ok(g)) { set_error("probav_gemm_conv3d_wgrad: bad geometry", hipSuccess); return PROBAV_EINVAL; }
    if (!gemm_wgrad_supported(g)) { set_error("probav_gemm_conv3d_wgrad: geometry not supported by the general matrix route", hipSuccess); return PROBAV_EINVAL; }
    if (scratch_bytes < gemm_wgrad_partial_floats(g) * sizeof(float)) { set_error("probav_gemm_conv3d_wgrad: scratch too small", hipSuccess); return PROBAV_ENOSPACE; }
    return gemm_conv_wgrad(g, x, dy, gate, dw, db, (float*)scratch, (hipStream_t)stream);
}

// What probav_plan_conv reports, for an engine with the route on: GEMM / WGRAD_GEMM where conv_route / wgrad_route of that engine's family hand the launch to the
// general matrix route, probav_plan_conv's answer everywhere else
int probav_plan_conv_gemm(const int32_t geom[17], int impl, int gated, int has_skip, int op, int32_t report[8])
{
    const int rc = probav_plan_conv(geom, impl, gated, has_skip, op, report);
    if (rc) return rc;
    const ConvGeom g = geom_from(geom);
    const Family f = make_family(impl, false, true);
    // (every filter fragment exists as far as the route can tell, as in op_conv_route: a geometry a matrix kernel serves stays with it)
    const Operands o = op_operands(gated != 0, op == PROBAV_PLAN_OP_FORWARD, has_skip != 0, impl);
    if (op == PROBAV_PLAN_OP_WGRAD) {
        if (wgrad_route(f, g, o).k != WgradKernel::gemm) return PROBAV_OK;
        int v[5];
        if (!gemm_wgrad_plan_ints(g, v)) return PROBAV_OK;
        for (int i = 0; i < 8; ++i) report[i] = 0;
        report[0] = PROBAV_PLAN_WGRAD_GEMM; report[1] = v[0]; report[2] = v[1]; report[3] = v[2]; report[4] = v[3]; report[5] = v[4];
        return PROBAV_OK;
    }
    if (report[0] != PROBAV_PLAN_NONE) return PROBAV_OK;       // a kernel serves the single-operator call (impl 0: direct; the dedicated upscale pair, which that call takes with a bias too)
    if (conv_route(f, g, o, true).k != ConvKernel::gemm) return PROBAV_OK;
    int v[6];
    if (!gemm_conv_plan_ints(g, v)) return PROBAV_OK;
    for (int i = 0; i < 8; ++i) report[i] = 0;
    report[0] = PROBAV_PLAN_GEMM; report[1] = v[3]; report[2] = v[2]; report[3] = v[0]; report[4] = v[1]; report[5] = v[2] * v[3]; report[6] = v[4]; report[7] = v[5];
    return PROBAV_OK;
}

// The x6 launches' plan for a geometry the route's kernels take: the fp32 route's tiles, grid and slabs under the x6 kernels' names
int probav_plan_conv_gemm_x6(const int32_t geom[17], int gated, int has_skip, int op, int32_t report[8])
{
    if (!geom || !report || op < PROBAV_PLAN_OP_FORWARD || op > PROBAV_PLAN_OP_WGRAD) { set_error("probav_plan_conv_gemm_x6: null/invalid argument", hipSuccess); return PROBAV_EINVAL; }
    const ConvGeom g = geom_from(geom);
    if (!geom_ok(g)) { set_error("probav_plan_conv_gemm_x6: bad geometry", hipSuccess); return PROBAV_EINVAL; }
    (void)gated; (void)has_skip;                                   // (one launch plan for every operand set: the gate is a select, bias and skip are the epilogue's)
    for (int i = 0; i < 8; ++i) report[i] = 0;
    if (op == PROBAV_PLAN_OP_WGRAD) return PROBAV_OK;            // no x6 kernel: the backward-filter stays the fp32 route's (probav_plan_conv_gemm reports it)
    int v[6];
    if (!gemm_x6_conv_plan_ints(g, v)) return PROBAV_OK;
    report[0] = PROBAV_PLAN_GEMM_X6; report[1] = v[3]; report[2] = v[2]; report[3] = v[0]; report[4] = v[1]; report[5] = v[2] * v[3]; report[6] = v[4]; report[7] = v[5];
    return PROBAV_OK;
}

// The route's plans for a wide geometry (what the fourth switch hands it): geom[17] has no field for the mirrored depth pad, so it is an argument.  x6: the report
// under the x6 kernel's name (the tiles are shared).  All zero for a geometry the wide predicates refuse
int probav_plan_conv_gemm_wide(const int32_t geom[17], int reflect_t, int x6, int op, int32_t report[8])
{
    if (!geom || !report || op < PROBAV_PLAN_OP_FORWARD || op > PROBAV_PLAN_OP_WGRAD) { set_error("probav_plan_conv_gemm_wide: null/invalid argument", hipSuccess); return PROBAV_EINVAL; }
    ConvGeom g = geom_from(geom);
    g.reflect_t = reflect_t != 0;
    for (int i = 0; i < 8; ++i) report[i] = 0;
    if (op == PROBAV_PLAN_OP_WGRAD) {
        int v[5];
        if (!gemm_wgrad_plan_ints_wide(g, v)) return PROBAV_OK;
        report[0] = PROBAV_PLAN_WGRAD_GEMM; report[1] = v[0]; report[2] = v[1]; report[3] = v[2]; report[4] = v[3]; report[5] = v[4];
        return PROBAV_OK;
    }
    int v[6];
    if (!(x6 ? gemm_x6_conv_plan_ints_wide(g, v) : gemm_conv_plan_ints_wide(g, v))) return PROBAV_OK;
    report[0] = x6 ? PROBAV_PLAN_GEMM_X6 : PROBAV_PLAN_GEMM; report[1] = v[3]; report[2] = v[2]; report[3] = v[0]; report[4] = v[1]; report[5] = v[2] * v[3]; report[6] = v[4]; report[7] = v[5];
    return PROBAV_OK;
}

size_t probav_gemm_wgrad_wide_scratch_bytes(const int32_t geom[17], int reflect_t)
{
    if (!geom) return 0;
    ConvGeom g = geom_from(geom);
    g.reflect_t = reflect_t != 0;
    if (!gemm_wgrad_supported_wide(g)) return 0;
    return gemm_wgrad_partial_floats(g) * sizeof(float);
}

// The launches of one training step by route: the launch list (step_launches), each entry routed as the passes route it
int probav_engine_route_counts(const probav_engine* e, int batch, int32_t counts[4])
{
    if (!e || !counts || batch < 1) { set_error("probav_engine_route_counts: null/invalid argument", hipSuccess); return PROBAV_EINVAL; }
    for (int i = 0; i < 4; ++i) counts[i] = 0;
    for (const Launch& L : step_launches(e, make_net(e, batch))) {
        const int slot = L.kind == LaunchKind::conv ? census_slot(conv_route(e->fam, L.g, L.o)) : (L.kind == LaunchKind::wgrad ? census_slot(wgrad_route(e->fam, L.g, L.o)) : -1);
        if (slot >= 0) ++counts[slot];
    }
    return PROBAV_OK;
}

// What the passes have actually launched since the last reset, counted where they launch (conv_fwd / conv_wgrad): the check of the census above
int probav_engine_launched_counts(probav_engine* e, int32_t counts[4], int reset)
{
    if (!e || !counts) { set_error("probav_engine_launched_counts: null argument", hipSuccess); return PROBAV_EINVAL; }
    for (int i = 0; i < 4; ++i) { counts[i] = e->launched[i]; if (reset) e->launched[i] = 0; }
    return PROBAV_OK;
}

int probav_plan_pw(int64_t nvox, int64_t vox_per_sample, int D, int impl, int backward, int32_t report[8])
{
    if (!report || nvox < 1 || impl < 2 || impl > 4) { set_error("probav_plan_pw: null/invalid argument", hipSuccess); return PROBAV_EINVAL; }
    for (int i = 0; i < 8; ++i) report[i] = 0;
    const long vps = vox_per_sample > 0 ? (long)vox_per_sample : (long)nvox;      // as probav_pw_forward / probav_pw_backward
    if (!mfma_pw_supported(32, 256, D) || nvox % vps) return PROBAV_OK;            // what those two refuse: no kernel
    if (impl == 2) { report[0] = PROBAV_PLAN_PW_MFMA; return PROBAV_OK; }
    static const int32_t fwd[4] = {PROBAV_PLAN_NONE, PROBAV_PLAN_PF4, PROBAV_PLAN_PW_H3K, PROBAV_PLAN_PW_X6};
    static const int32_t bwd[4] = {PROBAV_PLAN_NONE, PROBAV_PLAN_PW4, PROBAV_PLAN_PW_X6_H3, PROBAV_PLAN_PW_X6};
    int wps = 0;
    const int k = x6_pw_plan_kernel((long)nvox, vps, D, impl - 2, backward != 0, &wps);
    report[0] = backward ? bwd[k] : fwd[k];
    report[7] = wps;
    return PROBAV_OK;
}

int probav_wn_forward(probav_engine* e, const float* params, float* weff, float* weffT, float* inv_norm, void* stream)
{
    if (!e || !params || !weff || !weffT || !inv_norm) { set_error("probav_wn_forward: null argument", hipSuccess); return PROBAV_EINVAL; }
    CK(device_tables(e));
    return wn_forward(e->d_layers, (int)e->layers.size(), (int)e->cout_total, (int)e->cin_total, params, weff, weffT, inv_norm, nullptr, (hipStream_t)stream);
}
int probav_wn_backward(probav_engine* e, const float* params, const float* dweff, const float* inv_norm, float* grads, void* stream)
{
    if (!e || !params || !dweff || !inv_norm || !grads) { set_error("probav_wn_backward: null argument", hipSuccess); return PROBAV_EINVAL; }
    CK(device_tables(e));
    return wn_backward(e->d_layers, (int)e->layers.size(), (int)e->cout_total, params, dweff, inv_norm, grads, (hipStream_t)stream);
}

int probav_shift_loss_forward(const float* hr, const uint8_t* mask, const float* pred, int batch, int size, int border,
                              int bit_depth, float* l1, float* l2, float* cpsnr, int32_t* arg_l1, int32_t* arg_l2,
                              float* mean_l1, float* mean_l2, void* stream)
{
    if (!hr || !mask || !pred || !l1 || !l2 || !cpsnr || !arg_l1 || !arg_l2 || !mean_l1 || !mean_l2) {
        set_error("probav_shift_loss_forward: null argument", hipSuccess); return PROBAV_EINVAL;
    }
    const float maxv = (float)((1u << bit_depth) - 1u);        // Losses.numBytes = 2**bitDepth - 1 (models/loss.py:19)
    return shift_loss_forward(hr, mask, pred, batch, size, border, l1, l2, cpsnr, arg_l1, arg_l2, mean_l1, mean_l2, maxv, (hipStream_t)stream);
}
int probav_shift_loss_backward(const float* hr, const uint8_t* mask, const float* pred, const int32_t* arg, int batch, int size,
                               int border, int which, const float* upstream, float* dpred, void* stream)
{
    if (!hr || !mask || !pred || !arg || !dpred || batch < 1) { set_error("probav_shift_loss_backward: null argument", hipSuccess); return PROBAV_EINVAL; }
    return shift_loss_backward(hr, mask, pred, arg, batch, size, border, which, upstream, dpred, (hipStream_t)stream);
}
int probav_shift_l1edge_forward(const float* hr, const uint8_t* mask, const float* pred, int batch, int size, int border, float pi,
                                float* loss, int32_t* arg, float* mean, void* stream)
{
    if (!hr || !mask || !pred || !loss || !arg || !mean || batch < 1) { set_error("probav_shift_l1edge_forward: null argument", hipSuccess); return PROBAV_EINVAL; }
    return shift_l1edge_forward(hr, mask, pred, batch, size, border, pi, loss, arg, mean, mean + 1, (hipStream_t)stream);
}
int probav_shift_l1edge_backward(const float* hr, const uint8_t* mask, const float* pred, const int32_t* arg, int batch, int size,
                                 int border, float pi, const float* upstream, float* dpred, void* stream)
{
    if (!hr || !mask || !pred || !arg || !dpred || batch < 1) { set_error("probav_shift_l1edge_backward: null argument", hipSuccess); return PROBAV_EINVAL; }
    return shift_l1edge_backward(hr, mask, pred, arg, batch, size, border, pi, upstream, dpred, (hipStream_t)stream);
}
size_t probav_revssim_scratch_bytes(int batch, int border) { return batch > 0 && border >= 0 ? revssim_scratch_bytes(batch, border) : 0; }
int probav_revssim_forward(const float* hr, const uint8_t* mask, const float* pred, int batch, int size, int border, int bit_depth,
                           float eta, void* scratch, size_t scratch_bytes, float* loss, int32_t* arg, void* stream)
{
    if (!hr || !mask || !pred || !scratch || !loss || !arg || batch < 1) { set_error("probav_revssim_forward: null argument", hipSuccess); return PROBAV_EINVAL; }
    if (scratch_bytes < revssim_scratch_bytes(batch, border)) { set_error("probav_revssim_forward: scratch too small", hipSuccess); return PROBAV_ENOSPACE; }
    const float maxv = (float)((1u << bit_depth) - 1u);
    return revssim_forward(hr, mask, pred, batch, size, border, maxv, eta, (double*)scratch, loss, arg, (hipStream_t)stream);
}
int probav_revssim_backward(const float* hr, const uint8_t* mask, const float* pred, const int32_t* arg, const void* scratch, int batch,
                            int size, int border, int bit_depth, float eta, const float* upstream, float* dpred, void* stream)
{
    if (!hr || !mask || !pred || !arg || !scratch || !dpred || batch < 1) { set_error("probav_revssim_backward: null argument", hipSuccess); return PROBAV_EINVAL; }
    const float maxv = (float)((1u << bit_depth) - 1u);
    return revssim_backward(hr, mask, pred, arg, (const double*)scratch, batch, size, border, maxv, eta, upstream, dpred, (hipStream_t)stream);
}
int probav_nadam_step(float* params, const float* grads, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                      float eps, float c_g, float c_m, float c_v, void* stream)
{
    if (!params || !grads || !m || !v || n < 0) { set_error("probav_nadam_step: null/invalid argument", hipSuccess); return PROBAV_EINVAL; }
    return nadam_step(params, grads, m, v, (long)n, lr, beta1, beta2, eps, c_g, c_m, c_v, (hipStream_t)stream);
}
size_t probav_grad_guard_scratch_bytes(int64_t n) { return n < 0 ? 0 : grad_guard_scratch_bytes(); }
int probav_grad_guard(const float* grads, int64_t n, float clipnorm, int skip_nonfinite, void* scratch, size_t scratch_bytes, probav_guard_ctl* ctl, void* stream)
{
    if (!grads || !scratch || !ctl || n < 0) { set_error("probav_grad_guard: null/invalid argument", hipSuccess); return PROBAV_EINVAL; }
    if (clipnorm != clipnorm) { set_error("probav_grad_guard: clipnorm is NaN", hipSuccess); return PROBAV_EINVAL; }
    if (scratch_bytes < grad_guard_scratch_bytes()) { set_error("probav_grad_guard: scratch too small", hipSuccess); return PROBAV_ENOSPACE; }
    if (((uintptr_t)scratch & 7u) != 0) { set_error("probav_grad_guard: scratch must be 8-byte aligned", hipSuccess); return PROBAV_EINVAL; }
    return grad_guard(grads, (long)n, clipnorm, skip_nonfinite, (double*)scratch, ctl, (hipStream_t)stream);
}
int probav_nadam_step_guarded(float* params, const float* grads, float* m, float* v, float* ema, int64_t n, float lr, float beta1, float beta2,
                              float eps, float c_g, float c_m, float c_v, float ema_momentum, const probav_guard_ctl* ctl, void* stream)
{
    if (!params || !grads || !m || !v || n < 0) { set_error("probav_nadam_step_guarded: null/invalid argument", hipSuccess); return PROBAV_EINVAL; }
    if (ema && !(ema_momentum >= 0.f && ema_momentum <= 1.f)) { set_error("probav_nadam_step_guarded: ema_momentum outside [0, 1]", hipSuccess); return PROBAV_EINVAL; }
    return nadam_step_guarded(params, grads, m, v, ema, (long)n, lr, beta1, beta2, eps, c_g, c_m, c_v, ema_momentum, ctl, (hipStream_t)stream);
}

int probav_clip_round(const float* in, float* out, size_t n, float lo, float hi, void* stream)
{
    if (!in || !out) { set_error("probav_clip_round: null argument", hipSuccess); return PROBAV_EINVAL; }
    if (n == 0) return PROBAV_OK;
    return clip_round(in, out, n, lo, hi, (hipStream_t)stream);
}

}  // extern "C"
