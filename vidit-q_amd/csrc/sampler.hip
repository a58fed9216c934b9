// sampler.hip - the device-resident sampler steps for gfx950 (HBM-bound elementwise): fused classifier-free guidance +
// DDIM(eta=0) update (STDiT loop), and further down guidance + x0 + DPM-Solver++ multistep update and guidance +
// learned-range variance + ancestral (IDDPM) posterior step and guidance + x0 + SA-Solver corrector + predictor (PixArt
// loops).  The DPM-Solver++ step and the DDIM step also exist reading final_layer's patch-major output (the STDiT
// DPM-Solver++ loop; the STDiT DDIM loop in its table-driven form): one geometry walk, patch_walk, serves both.
//
// Replaces, for the first (kept) half of the duplicated batch, the tail of forward_with_cfg
// (t2v/opensora/schedulers/iddpm/__init__.py:168-184: PTQD division, CFG on eps[:, :3] only) and
// p_mean_variance + ddim_sample (iddpm/gaussian_diffusion.py:252-335, 514-552) with eta = 0:
//   e      = c<3 ? u + cfg*(cnd - u) : cnd            (each first divided by 1+k)
//   x0     = A*x - Bc*e                               (_predict_xstart_from_eps)
//   e2     = (A*x - x0) / Bc                          (_predict_eps_from_xstart)
//   x_next = x0*sqrt(abar_prev) + sqrt(1 - abar_prev)*e2
// cond/uncond: fp32 [n, 2C, inner] model outputs; x, x_out: fp32 [n, C, inner].
#include "vq_common.h"

__global__ __launch_bounds__(256) void cfg_ddim_kernel(const float* __restrict__ cond, const float* __restrict__ unc,
                                                       const float* __restrict__ x, float* __restrict__ xo, int n,
                                                       int Cc, long inner, float cfg, float one_plus_k, float A,
                                                       float Bc, float abar_prev) {
    const long total = (long)n * Cc * inner;
    const float sa = __fsqrt_rn(abar_prev), sb = __fsqrt_rn(1.0f - abar_prev - 0.0f);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long in_ = i % inner;
        const int c = (int)((i / inner) % Cc);
        const long b = i / (inner * Cc);
        const long mo = (b * 2 * Cc + c) * inner + in_;
        const float cv = __fdiv_rn(cond[mo], one_plus_k);
        const float uv = __fdiv_rn(unc[mo], one_plus_k);
        const float e = c < 3 ? uv + cfg * (cv - uv) : cv;
        const float xv = x[i];
        const float x0 = A * xv - Bc * e;
        const float e2 = __fdiv_rn(A * xv - x0, Bc);
        xo[i] = x0 * sa + sb * e2;
    }
}

extern "C" int vq_cfg_ddim_step(const float* cond, const float* uncond, const float* x, float* x_out, int n, int C,
                                int inner, float cfg, float one_plus_k, float A, float Bc, float abar_prev,
                                void* stream) {
    if (!cond || !uncond || !x || !x_out || n <= 0 || C <= 0 || inner <= 0) return VQ_EINVAL;
    const long total = (long)n * C * inner;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(cfg_ddim_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, cond, uncond, x, x_out, n, C,
                       (long)inner, cfg, one_plus_k, A, Bc, abar_prev);
    return vq_check_launch();
}

// ---- fused CFG + data-prediction DPM-Solver++ multistep update (the PixArt sampling loop) ---------------------------
// One launch per model call k of t2i/diffusion/model/dpm_solver_sigma.py: model_wrapper's guidance (:318-332),
// data_prediction_fn (:435-444) and dpm_solver_first_update (:551-596) / multistep_dpm_solver_second_update (:805-862) /
// multistep_dpm_solver_third_update (:864-915).  Row layout and contract: include/viditq.h (vq_cfg_dpmpp_step).
// Every operation is rounded on its own, as the eager torch expressions round it: no contraction (the pragma below; -O3
// would otherwise fuse a*x - b*m into an fma), and with an fp16 model the four fp16 roundings of c - u, cfg * (.),
// u + (.) and sigma_t * e.  The division by alpha_t is the product with the fp32 reciprocal the row holds (what torch's
// GPU division by a host scalar computes).
typedef __attribute__((ext_vector_type(2))) _Float16 half2v;
template <typename T, int V> struct dpm_vec;
template <> struct dpm_vec<float, 4> { typedef float4v type; };
template <> struct dpm_vec<float, 2> { typedef float2v type; };
template <> struct dpm_vec<float, 1> { typedef float type; };
template <> struct dpm_vec<half_t, 4> { typedef half4 type; };
template <> struct dpm_vec<half_t, 2> { typedef half2v type; };
template <> struct dpm_vec<half_t, 1> { typedef half_t type; };

template <typename T, int V>
__device__ __forceinline__ void dpm_load(const T* p, float (&v)[V]) {
    typename dpm_vec<T, V>::type r = *reinterpret_cast<const typename dpm_vec<T, V>::type*>(p);
    if constexpr (V == 1) {
        v[0] = (float)r;
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = (float)r[j];
    }
}

template <typename T, int V>
__device__ __forceinline__ void dpm_store(T* p, const float (&v)[V]) {
    typename dpm_vec<T, V>::type r;
    if constexpr (V == 1) {
        r = (T)v[0];
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) r[j] = (T)v[j];
    }
    *reinterpret_cast<typename dpm_vec<T, V>::type*>(p) = r;
}

// What the table-driven step kernels (DPM-Solver++ here, IDDPM and SA-Solver further down) share.  The contract pragma is scoped to
// a function body: a helper with floating-point arithmetic carries its own.

// The table row of a launch: ``row`` plus the device counter when there is one.
__device__ __forceinline__ int step_row(int row, const int32_t* step, int n_rows) {
    const int k = row + (step ? *step : 0);
    return k < 0 ? 0 : (k < n_rows - 1 ? k : n_rows - 1);       // a counter can never index outside the table
}

// Classifier-free guidance u + cfg * (c - u) as the eager tensors round it: each of the three operations in the model
// output's type T.  Returns e as a float that is exactly the fp16 value when T is half_t.
template <typename T>
__device__ __forceinline__ float step_guide(float c, float u, float cfg) {
#pragma clang fp contract(off)
    const T d = (T)(c - u);
    const T p = (T)(cfg * (float)d);
    return (float)(T)(u + (float)p);
}

// The sample for the next forward: both halves of the duplicated batch x_model, in its own type.
template <int V>
__device__ __forceinline__ void step_store_model(void* xm, int xm_f16, long i, long total, const float (&out)[V]) {
    if (!xm) return;
    if (xm_f16) {
        dpm_store<half_t, V>((half_t*)xm + i, out);
        dpm_store<half_t, V>((half_t*)xm + total + i, out);
    } else {
        dpm_store<float, V>((float*)xm + i, out);
        dpm_store<float, V>((float*)xm + total + i, out);
    }
}

// The coefficient row of a DPM-Solver++ launch, read once per thread.
struct dpmpp_row {
    int order;
    bool taylor;
    float cfg, sigma, inv_alpha, a, b, c1, c2, ir0, ir1, f, g;
};

__device__ __forceinline__ dpmpp_row dpmpp_load_row(const float* __restrict__ coef, int k) {
    const float* r = coef + (long)k * VQ_DPMPP_ROW;
    dpmpp_row R;
    R.order = (int)r[VQ_DPMPP_ORDER];
    R.taylor = r[VQ_DPMPP_TAYLOR] != 0.0f;
    R.cfg = r[VQ_DPMPP_CFG], R.sigma = r[VQ_DPMPP_SIGMA], R.inv_alpha = r[VQ_DPMPP_INV_ALPHA];
    R.a = r[VQ_DPMPP_X], R.b = r[VQ_DPMPP_M0], R.c1 = r[VQ_DPMPP_D1], R.c2 = r[VQ_DPMPP_D2];
    R.ir0 = r[VQ_DPMPP_INV_R0], R.ir1 = r[VQ_DPMPP_INV_R1], R.f = r[VQ_DPMPP_R0_FRAC], R.g = r[VQ_DPMPP_INV_R01];
    return R;
}

// Guidance, x0 and the order 1 / 2 / 3 update of one element (the body both DPM-Solver++ kernels share).  T: the type the
// eager tensors round the guidance and sigma_t * e in (half_t for an fp16 model output used as it is, float for one that
// was widened first).  m1 / m2 are read for orders >= 2 / >= 3 only.  Returns x_out; m0 receives m_k.
template <typename T>
__device__ __forceinline__ float dpmpp_element(const dpmpp_row& R, float c, float u, float xv, float m1, float m2, float& m0) {
#pragma clang fp contract(off)
    const float e = step_guide<T>(c, u, R.cfg);
    const float se = (float)(T)(R.sigma * e);
    const float t = xv - se;
    const float m = t * R.inv_alpha;
    m0 = m;
    const float ax = R.a * xv;
    const float bm = R.b * m;
    float o = ax - bm;
    if (R.order == 2) {
        const float dm = m - m1;
        const float D1_0 = R.ir0 * dm;
        const float cd = R.c1 * D1_0;
        o = R.taylor ? o + cd : o - cd;
    } else if (R.order >= 3) {
        const float dm0 = m - m1;
        const float D1_0 = R.ir0 * dm0;
        const float dm1 = m1 - m2;
        const float D1_1 = R.ir1 * dm1;
        const float dd = D1_0 - D1_1;
        const float fd = R.f * dd;
        const float D1 = D1_0 + fd;
        const float D2 = R.g * dd;
        const float p2 = R.c1 * D1;
        const float p3 = R.c2 * D2;
        o = o + p2;
        o = o - p3;
    }
    return o;
}

// T: the model output's type; V: elements per thread and access (4 needs inner % 4 == 0, so a group never spans two
// batch elements).  x_out may alias x: an element is read and written by the same thread.
template <typename T, int V>
__global__ __launch_bounds__(256) void cfg_dpmpp_kernel(const T* __restrict__ eps, const float* x, float* hist,
                                                        const float* __restrict__ coef, const int32_t* __restrict__ step,
                                                        float* xo, void* xm, int xm_f16, int n, long CI, long ld_eps,
                                                        int row, int n_rows) {
    const int k = step_row(row, step, n_rows);
    const dpmpp_row R = dpmpp_load_row(coef, k);
    const long total = (long)n * CI;
    float* h0 = hist + (long)(k % 3) * total;                    // written: m_k
    const float* h1 = hist + (long)((k + 2) % 3) * total;        // m_{k-1}
    const float* h2 = hist + (long)((k + 1) % 3) * total;        // m_{k-2}
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * V; i < total; i += (long)gridDim.x * blockDim.x * V) {
        const long bi = i / CI, ri = i - bi * CI;
        float u[V], c[V], xv[V], m1[V] = {}, m2[V] = {}, m0[V], out[V];
        dpm_load<T, V>(eps + bi * ld_eps + ri, u);
        dpm_load<T, V>(eps + (bi + n) * ld_eps + ri, c);
        dpm_load<float, V>(x + i, xv);
        if (R.order >= 2) dpm_load<float, V>(h1 + i, m1);
        if (R.order >= 3) dpm_load<float, V>(h2 + i, m2);
#pragma unroll
        for (int j = 0; j < V; ++j) out[j] = dpmpp_element<T>(R, c[j], u[j], xv[j], m1[j], m2[j], m0[j]);
        dpm_store<float, V>(h0 + i, m0);
        dpm_store<float, V>(xo + i, out);
        step_store_model<V>(xm, xm_f16, i, total, out);
    }
}

static inline bool vq_aligned(const void* p, size_t a) { return p == nullptr || ((uintptr_t)p % a) == 0; }

// The refusals of the step entry points, in the order include/viditq.h documents: VQ_EINVAL (``einval``: the solver's own
// nulls and ranges; then what both have), VQ_ESHAPE (an element of elem_mult * C * inner values within the pitch and the
// solver's clause ``eshape``; then the pitch and every address on the V elements of an access: ``f32`` is the
// null-terminated list of the fp32 operands moved V at a time, of which an optional one may only stand last), VQ_EUNSUP
// (a flag outside {0, 1}).  Sets V and returns VQ_OK when the launch may go ahead.
static int step_check(bool einval, bool eshape, const void* eps, const void* const* f32, const float* coef,
                      const int32_t* step, const void* x_model, int n, int C, int inner, long ld_eps, int elem_mult, int row,
                      int n_rows, int eps_f16, int xm_f16, int* V_out) {
    if (einval || !eps || !coef || n <= 0 || C <= 0 || inner <= 0 || row < 0 || n_rows <= 0 || row >= n_rows) return VQ_EINVAL;
    if (ld_eps < elem_mult * (long)C * inner || eshape) return VQ_ESHAPE;
    const int V = *V_out = inner % 4 == 0 ? 4 : 1;
    const bool e16 = eps_f16 == 1, m16 = xm_f16 == 1;            // (a flag outside {0, 1} is refused below, after the shapes)
    bool aligned = ld_eps % V == 0 && vq_aligned(eps, (e16 ? 2 : 4) * V) && vq_aligned(x_model, (m16 ? 2 : 4) * V) &&
                   vq_aligned(coef, 4) && vq_aligned(step, 4);
    for (; *f32; ++f32) aligned = aligned && vq_aligned(*f32, 4 * V);
    if (!aligned) return VQ_ESHAPE;
    if (eps_f16 < 0 || eps_f16 > 1 || xm_f16 < 0 || xm_f16 > 1) return VQ_EUNSUP;
    return VQ_OK;
}

// One launch of a step kernel template over n * CI elements: ``launch(T(), V, grid)`` is called with the model output's
// type as a value and V as an integral constant, once.
template <typename F>
static int step_launch(int n, long CI, int V, int eps_f16, F launch) {
    const long total = (long)n * CI;
    long blocks = ((total + V - 1) / V + 255) / 256;
    if (blocks > 1024) blocks = 1024;                            // 16 waves per CU in flight; larger latents loop
    const dim3 grid((unsigned)blocks);
    typedef std::integral_constant<int, 4> four;
    typedef std::integral_constant<int, 1> one;
    if (eps_f16) {
        if (V == 4) launch(half_t(), four(), grid); else launch(half_t(), one(), grid);
    } else {
        if (V == 4) launch(float(), four(), grid); else launch(float(), one(), grid);
    }
    return vq_check_launch();
}

extern "C" int vq_cfg_dpmpp_step(const void* eps, const float* x, float* hist, const float* coef, const int32_t* step,
                                 float* x_out, void* x_model, int n, int C, int inner, long ld_eps, int row, int n_rows,
                                 int eps_f16, int xm_f16, void* stream) {
    const void* const f32[] = {x, hist, x_out, nullptr};
    int V;
    const int rc = step_check(!x || !hist || !x_out, false, eps, f32, coef, step, x_model, n, C, inner, ld_eps, 1, row, n_rows,
                              eps_f16, xm_f16, &V);
    if (rc != VQ_OK) return rc;
    const long CI = (long)C * inner;
    return step_launch(n, CI, V, eps_f16, [&](auto t, auto v, dim3 grid) {
        typedef decltype(t) T;
        hipLaunchKernelGGL((cfg_dpmpp_kernel<T, decltype(v)::value>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)eps,
                           x, hist, coef, step, x_out, x_model, xm_f16, n, CI, ld_eps, row, n_rows);
    });
}

// ---- the same step reading final_layer's patch-major output (the STDiT sampling loop) -------------------------------
// eps_u / eps_c: [n, N_t*N_h*N_w tokens, p_t*p_h*p_w*C_out columns], sample pitch ld_eps; latent element (b, c, t, h, w) is
// at token ((t/p_t)*N_h + h/p_h)*N_w + w/p_w, column (((t%p_t)*p_h + h%p_h)*p_w + w%p_w)*C_out + c (STDiT.unpatchify).
// Every value is widened to fp32 on load and the arithmetic is dpmpp_element<float>: what unpatchify, .to(float32) and
// the eager fp32 expressions compute.  Patch extents are 1 or 2 and are passed as shifts.
struct patch_geo {
    int C, C_out, T, H, W;                       // latent channels read, channels per patch position, latent extents
    int lt, lh, lw;                              // log2 of the patch extents
    long ld_eps;
};

// VC x VW: channels per eps access x elements along w per fp32 access.  4 x 2 (C == 4: one thread owns the four channels
// of two neighbouring w, the eps reads are 8 / 16 bytes and the dense streams run along w) or 1 x 1 (any C: one element per
// thread).
//
// The geometry walk of the patch-major step kernels (owner: this helper; both kernels below call it).  One item is VC
// channels x VW neighbouring w of one (b, t, h); the grid-stride loop hands each to
//   item(b, c0, t, h, w0, e, i):  e[j] the offset of (b, c0, t, h, w0 + j) in a model output, i the dense offset of
//                                 (b, c0, t, h, w0) in [n, C, T, H, W]; channel c0 + cc is at i + cc * T*H*W.
// An element is read and written by the same thread, so a dense output may alias a dense input.
template <int VC, int VW, typename F>
__device__ __forceinline__ void patch_walk(int n, const patch_geo& g, F item) {
    const long HW = (long)g.H * g.W;
    const int Wg = g.W / VW, Cg = VC == 1 ? g.C : 1;             // (VC == 4: the channels are inside the item)
    const int Nh = g.H >> g.lh, Nw = g.W >> g.lw, ph = 1 << g.lh, pw = 1 << g.lw;
    const long PC = (long)(1 << (g.lt + g.lh + g.lw)) * g.C_out; // columns of a token
    const long items = (long)n * Cg * g.T * g.H * Wg;
    for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (long)gridDim.x * blockDim.x) {
        long r = it;
        const int w0 = (int)(r % Wg) * VW;  r /= Wg;
        const int h = (int)(r % g.H);       r /= g.H;
        const int t = (int)(r % g.T);       r /= g.T;
        const int c0 = (int)(r % Cg);       r /= Cg;
        const long b = r;
        const long tok = ((long)(t >> g.lt) * Nh + (h >> g.lh)) * Nw;
        const int pos = ((t & ((1 << g.lt) - 1)) * ph + (h & (ph - 1))) * pw;
        long e[VW];
#pragma unroll
        for (int j = 0; j < VW; ++j) {
            const int w = w0 + j;
            e[j] = b * g.ld_eps + (tok + (w >> g.lw)) * PC + (long)(pos + (w & (pw - 1))) * g.C_out + c0;
        }
        item(b, c0, t, h, w0, e, ((b * g.C + c0) * g.T + t) * HW + (long)h * g.W + w0);
    }
}

// The uncond and the cond values of one item, widened to fp32.
template <typename T, int VC, int VW>
__device__ __forceinline__ void patch_load(const T* __restrict__ eps_u, const T* __restrict__ eps_c, const long (&e)[VW],
                                           float (&u)[VW][VC], float (&c)[VW][VC]) {
#pragma unroll
    for (int j = 0; j < VW; ++j) {
        dpm_load<T, VC>(eps_u + e[j], u[j]);
        dpm_load<T, VC>(eps_c + e[j], c[j]);
    }
}

// The sample for the next forward(s): xm_copies times [n, C, T, H, W] in x_model's own type.
template <int VW>
__device__ __forceinline__ void patch_store_model(void* xm, int xm_f16, int xm_copies, long total, long i,
                                                  const float (&out)[VW]) {
    for (int q = 0; q < (xm ? xm_copies : 0); ++q) {
        if (xm_f16) dpm_store<half_t, VW>((half_t*)xm + q * total + i, out);
        else dpm_store<float, VW>((float*)xm + q * total + i, out);
    }
}

// x_out may alias x (patch_walk).
template <typename T, int VC, int VW>
__global__ __launch_bounds__(256) void cfg_dpmpp_patch_kernel(const T* __restrict__ eps_u, const T* __restrict__ eps_c,
                                                              const float* x, float* hist, const float* __restrict__ coef,
                                                              const int32_t* __restrict__ step, float* xo, void* xm,
                                                              int xm_f16, int xm_copies, int n, patch_geo g, int row,
                                                              int n_rows) {
    const int k = step_row(row, step, n_rows);
    const dpmpp_row R = dpmpp_load_row(coef, k);
    const long CS = (long)g.T * g.H * g.W, total = (long)n * g.C * CS;
    float* h0 = hist + (long)(k % 3) * total;                    // written: m_k
    const float* h1 = hist + (long)((k + 2) % 3) * total;        // m_{k-1}
    const float* h2 = hist + (long)((k + 1) % 3) * total;        // m_{k-2}
    patch_walk<VC, VW>(n, g, [&](long, int, int, int, int, const long (&e)[VW], long i0) {
        float u[VW][VC], c[VW][VC];
        patch_load<T, VC, VW>(eps_u, eps_c, e, u, c);
#pragma unroll
        for (int cc = 0; cc < VC; ++cc) {
            const long i = i0 + cc * CS;
            float xv[VW], m1[VW] = {}, m2[VW] = {}, m0[VW], out[VW];
            dpm_load<float, VW>(x + i, xv);
            if (R.order >= 2) dpm_load<float, VW>(h1 + i, m1);
            if (R.order >= 3) dpm_load<float, VW>(h2 + i, m2);
#pragma unroll
            for (int j = 0; j < VW; ++j) out[j] = dpmpp_element<float>(R, c[j][cc], u[j][cc], xv[j], m1[j], m2[j], m0[j]);
            dpm_store<float, VW>(h0 + i, m0);
            dpm_store<float, VW>(xo + i, out);
            patch_store_model<VW>(xm, xm_f16, xm_copies, total, i, out);
        }
    });
}

static inline int vq_log2_patch(int p) { return p == 1 ? 0 : (p == 2 ? 1 : -1); }

// The refusals of the patch-major entry points, in the order include/viditq.h documents: VQ_EINVAL (``einval``: the
// solver's own nulls and ranges; then what both have), VQ_ESHAPE (the shapes, the pitch, then every address on the elements
// of an access: ``f32`` is the null-terminated list of the dense fp32 operands, of which an optional one may only stand
// last), VQ_EUNSUP (a patch extent outside {1, 2}, a flag outside {0, 1}, xm_copies outside {1, 2}).  Sets the geometry,
// the access form and the grid, and returns VQ_OK when the launch may go ahead.
static int patch_check(bool einval, const void* eps_u, const void* eps_c, const void* const* f32, const float* coef,
                       const int32_t* step, const void* x_model, int n, int C, int C_out, int T, int H, int W, int p_t,
                       int p_h, int p_w, long ld_eps, int row, int n_rows, int eps_f16, int xm_f16, int xm_copies,
                       patch_geo* g_out, bool* wide_out, dim3* grid_out) {
    if (einval || !eps_u || !eps_c || !coef || n <= 0 || C <= 0 || C_out <= 0 || T <= 0 || H <= 0 || W <= 0 || p_t <= 0 ||
        p_h <= 0 || p_w <= 0 || row < 0 || n_rows <= 0 || row >= n_rows)
        return VQ_EINVAL;
    if (C > C_out || T % p_t || H % p_h || W % p_w) return VQ_ESHAPE;
    // one sample of the model output: T*H*W positions (tokens x patch positions) of C_out columns each
    if (ld_eps < (long)T * H * W * C_out) return VQ_ESHAPE;
    const bool wide = *wide_out = C == 4 && C_out % 4 == 0 && W % 2 == 0;
    const int VC = wide ? 4 : 1, VW = wide ? 2 : 1;
    const size_t e_sz = eps_f16 == 1 ? 2 : 4, m_sz = xm_f16 == 1 ? 2 : 4;     // (a flag outside {0, 1} is refused below)
    bool aligned = ld_eps % VC == 0 && vq_aligned(eps_u, e_sz * VC) && vq_aligned(eps_c, e_sz * VC) &&
                   vq_aligned(x_model, m_sz * VW) && vq_aligned(coef, 4) && vq_aligned(step, 4);
    for (; *f32; ++f32) aligned = aligned && vq_aligned(*f32, 4 * VW);
    if (!aligned) return VQ_ESHAPE;
    patch_geo& g = *g_out;
    g.C = C, g.C_out = C_out, g.T = T, g.H = H, g.W = W, g.ld_eps = ld_eps;
    g.lt = vq_log2_patch(p_t), g.lh = vq_log2_patch(p_h), g.lw = vq_log2_patch(p_w);
    if (g.lt < 0 || g.lh < 0 || g.lw < 0 || eps_f16 < 0 || eps_f16 > 1 || xm_f16 < 0 || xm_f16 > 1 || xm_copies < 1 ||
        xm_copies > 2)
        return VQ_EUNSUP;
    const long items = (long)n * (wide ? 1 : C) * T * H * (W / VW);
    long blocks = (items + 255) / 256;
    if (blocks > 1024) blocks = 1024;                            // 16 waves per CU in flight; larger latents loop
    *grid_out = dim3((unsigned)blocks);
    return VQ_OK;
}

// One launch of a patch-major kernel template: ``launch(T(), VC, VW)`` is called once, with the model output's type as a
// value and the access form as integral constants.
template <typename F>
static int patch_launch(bool wide, int eps_f16, F launch) {
    typedef std::integral_constant<int, 4> four;
    typedef std::integral_constant<int, 2> two;
    typedef std::integral_constant<int, 1> one;
    if (eps_f16) {
        if (wide) launch(half_t(), four(), two()); else launch(half_t(), one(), one());
    } else {
        if (wide) launch(float(), four(), two()); else launch(float(), one(), one());
    }
    return vq_check_launch();
}

extern "C" int vq_cfg_dpmpp_step_patch(const void* eps_u, const void* eps_c, const float* x, float* hist, const float* coef,
                                       const int32_t* step, float* x_out, void* x_model, int n, int C, int C_out, int T, int H,
                                       int W, int p_t, int p_h, int p_w, long ld_eps, int row, int n_rows, int eps_f16,
                                       int xm_f16, int xm_copies, void* stream) {
    const void* const f32[] = {x, hist, x_out, nullptr};
    patch_geo g;
    bool wide;
    dim3 grid;
    const int rc = patch_check(!x || !hist || !x_out, eps_u, eps_c, f32, coef, step, x_model, n, C, C_out, T, H, W, p_t, p_h,
                               p_w, ld_eps, row, n_rows, eps_f16, xm_f16, xm_copies, &g, &wide, &grid);
    if (rc != VQ_OK) return rc;
    return patch_launch(wide, eps_f16, [&](auto t, auto vc, auto vw) {
        typedef decltype(t) T_;
        hipLaunchKernelGGL((cfg_dpmpp_patch_kernel<T_, decltype(vc)::value, decltype(vw)::value>), grid, dim3(256), 0,
                           (hipStream_t)stream, (const T_*)eps_u, (const T_*)eps_c, x, hist, coef, step, x_out, x_model,
                           xm_f16, xm_copies, n, g, row, n_rows);
    });
}

// ---- the DDIM(eta = 0) step of the STDiT loop on the same patch-major output, table-driven --------------------------
// Contract and operation sequence: include/viditq.h (vq_cfg_ddim_step_patch).  The row of a launch, read once per thread;
// the two square roots are cfg_ddim_kernel's expressions.
struct ddim_row {
    float cfg, opk, A, Bc, sa, sb;
};

__device__ __forceinline__ ddim_row ddim_load_row(const float* __restrict__ coef, int k) {
    const float* r = coef + (long)k * VQ_DDIM_ROW;
    ddim_row R;
    R.cfg = r[VQ_DDIM_CFG], R.opk = r[VQ_DDIM_ONE_PLUS_K], R.A = r[VQ_DDIM_A], R.Bc = r[VQ_DDIM_BC];
    const float abp = r[VQ_DDIM_ABAR_PREV];
    R.sa = __fsqrt_rn(abp), R.sb = __fsqrt_rn(1.0f - abp - 0.0f);
    return R;
}

// vq_cfg_ddim_step's kernel covers 4096 x 256 elements per pass of its grid-stride loop, and its compiled form rounds an
// element in one of two ways (include/viditq.h): ``paired`` for the passes a thread takes two at a time, the other for a
// thread's odd last pass - which is every element of a latent of up to 2^20 elements.  Which way element i of ``total`` goes:
__device__ __forceinline__ bool ddim_paired(long i, long total) {
    const long pass = 1L << 20;
    if (total <= pass) return false;
    const long first = i & (pass - 1);                           // the thread's first element
    const long passes = ((total - 1 - first) >> 20) + 1;         // how many that thread takes
    return (i >> 20) < (passes & ~1L);
}

// One element: PTQD division, guidance on the channels below ``guided``, x0, eps back from x0 and the eta = 0 update,
// every operation spelled out.  Under the pragma a plain * / - / + is one rounding and is never fused; every fused
// multiply-add is an explicit __fmaf_rn.  (The __fmul_rn / __fsub_rn / __fadd_rn intrinsics are NOT used for the unfused
// operations: they are inline header functions compiled in the header's contraction mode, and hipcc fuses a product and a
// sum written through them - measured here, where both forms of ``r`` came out as one v_fma_f32.)
__device__ __forceinline__ float ddim_element(const ddim_row& R, float cnd, float unc, float xv, bool guide, bool paired) {
#pragma clang fp contract(off)
    const float cv = __fdiv_rn(cnd, R.opk);
    const float uv = __fdiv_rn(unc, R.opk);
    const float d = cv - uv;
    const float e = guide ? __fmaf_rn(R.cfg, d, uv) : cv;
    const float be = R.Bc * e;
    const float x0 = __fmaf_rn(R.A, xv, -be);
    const float ax = R.A * xv;
    const float r = paired ? __fmaf_rn(R.A, xv, -x0) : ax - x0;
    const float e2 = __fdiv_rn(r, R.Bc);
    const float p2 = R.sb * e2;
    const float p1 = R.sa * x0;
    return paired ? __fmaf_rn(R.sa, x0, p2) : p1 + p2;
}

template <typename T, int VC, int VW>
__global__ __launch_bounds__(256) void cfg_ddim_patch_kernel(const T* __restrict__ eps_c, const T* __restrict__ eps_u,
                                                             const float* x, const float* __restrict__ coef,
                                                             const int32_t* __restrict__ step, float* xo, void* xm,
                                                             int xm_f16, int xm_copies, int n, patch_geo g, int guided,
                                                             int row, int n_rows) {
    const ddim_row R = ddim_load_row(coef, step_row(row, step, n_rows));
    const long CS = (long)g.T * g.H * g.W, total = (long)n * g.C * CS;
    patch_walk<VC, VW>(n, g, [&](long, int c0, int, int, int, const long (&e)[VW], long i0) {
        float u[VW][VC], c[VW][VC];
        patch_load<T, VC, VW>(eps_u, eps_c, e, u, c);
#pragma unroll
        for (int cc = 0; cc < VC; ++cc) {
            const long i = i0 + cc * CS;
            float xv[VW], out[VW];
            dpm_load<float, VW>(x + i, xv);
#pragma unroll
            for (int j = 0; j < VW; ++j)
                out[j] = ddim_element(R, c[j][cc], u[j][cc], xv[j], c0 + cc < guided, ddim_paired(i + j, total));
            dpm_store<float, VW>(xo + i, out);
            patch_store_model<VW>(xm, xm_f16, xm_copies, total, i, out);
        }
    });
}

extern "C" int vq_cfg_ddim_step_patch(const void* eps_c, const void* eps_u, const float* x, const float* coef,
                                      const int32_t* step, float* x_out, void* x_model, int n, int C, int C_out, int T, int H,
                                      int W, int p_t, int p_h, int p_w, long ld_eps, int guided, int row, int n_rows,
                                      int eps_f16, int xm_f16, int xm_copies, void* stream) {
    const void* const f32[] = {x, x_out, nullptr};
    patch_geo g;
    bool wide;
    dim3 grid;
    const int rc = patch_check(!x || !x_out || guided < 0, eps_u, eps_c, f32, coef, step, x_model, n, C, C_out, T, H, W, p_t,
                               p_h, p_w, ld_eps, row, n_rows, eps_f16, xm_f16, xm_copies, &g, &wide, &grid);
    if (rc != VQ_OK) return rc;
    return patch_launch(wide, eps_f16, [&](auto t, auto vc, auto vw) {
        typedef decltype(t) T_;
        hipLaunchKernelGGL((cfg_ddim_patch_kernel<T_, decltype(vc)::value, decltype(vw)::value>), grid, dim3(256), 0,
                           (hipStream_t)stream, (const T_*)eps_c, (const T_*)eps_u, x, coef, step, x_out, x_model, xm_f16,
                           xm_copies, n, g, guided, row, n_rows);
    });
}

// One workgroup, after the step kernel in stream order: t_out[0 .. n_t) = the row's next model-input time, then the
// counter moves on (saturating).  Every thread reads the counter before the barrier; thread 0 writes it after.
__global__ __launch_bounds__(256) void dpmpp_advance_kernel(int32_t* step, const float* __restrict__ coef, int n_rows,
                                                            float* __restrict__ t_out, int n_t) {
    int k = *step;
    k = k < 0 ? 0 : (k < n_rows - 1 ? k : n_rows - 1);
    const float t = coef[(long)k * VQ_DPMPP_ROW + VQ_DPMPP_T_NEXT];
    for (int i = threadIdx.x; i < n_t; i += blockDim.x) t_out[i] = t;
    __syncthreads();
    if (threadIdx.x == 0) *step = k < n_rows - 1 ? k + 1 : n_rows - 1;
}

extern "C" int vq_dpmpp_advance(int32_t* step, const float* coef, int n_rows, float* t_out, int n_t, void* stream) {
    if (!step || !coef || !t_out || n_rows <= 0 || n_t <= 0) return VQ_EINVAL;
    if (!vq_aligned(step, 4) || !vq_aligned(coef, 4) || !vq_aligned(t_out, 4)) return VQ_ESHAPE;
    hipLaunchKernelGGL(dpmpp_advance_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, step, coef, n_rows, t_out, n_t);
    return vq_check_launch();
}

// ---- fused CFG + learned-range variance + ancestral posterior step (the PixArt IDDPM sampling loop) -----------------
// One launch per model call of p_sample_loop(model.forward_with_cfg, ...): the tail of forward_with_cfg
// (t2i/diffusion/model/nets/PixArtMS.py:221-234), p_mean_variance (t2i/diffusion/model/gaussian_diffusion.py:303-318),
// _predict_xstart_from_eps (:363-368), q_posterior_mean_variance (:264-267) and p_sample (:439-445) for the kept first half
// of the duplicated batch.  Row layout and contract: include/viditq.h (vq_cfg_ddpm_step).  As above nothing is contracted
// and an fp16 model output gets the fp16 roundings of the eager tensors: c - u, cfg * (.), u + (.), v + 1, (.) * 0.5 and
// 1 - frac; whatever meets a coefficient is fp32.  exp is the library expf.
template <typename T, int V>
__global__ __launch_bounds__(256) void cfg_ddpm_kernel(const T* __restrict__ eps, const float* x,
                                                       const float* __restrict__ noise, const float* __restrict__ coef,
                                                       const int32_t* __restrict__ step, float* xo, float* x0o, void* xm,
                                                       int xm_f16, int n, long inner, long CI, long ld_eps, int guided,
                                                       int row, int n_rows) {
#pragma clang fp contract(off)
    const float* r = coef + (long)step_row(row, step, n_rows) * VQ_DDPM_ROW;
    const float cfg = r[VQ_DDPM_CFG], A = r[VQ_DDPM_A], B = r[VQ_DDPM_B], c1 = r[VQ_DDPM_C1], c2 = r[VQ_DDPM_C2];
    const float min_log = r[VQ_DDPM_MIN_LOG], max_log = r[VQ_DDPM_MAX_LOG], nonzero = r[VQ_DDPM_NONZERO];
    const bool clip = r[VQ_DDPM_CLIP] != 0.0f;
    const long total = (long)n * CI;
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * V; i < total; i += (long)gridDim.x * blockDim.x * V) {
        const long bi = i / CI, ri = i - bi * CI;
        const bool guide = ri / inner < guided;                  // V == 4 has inner % 4 == 0: a group lies in one channel
        float c[V], u[V], v[V], xv[V], z[V], x0[V], out[V];
        dpm_load<T, V>(eps + bi * ld_eps + ri, c);
        dpm_load<T, V>(eps + bi * ld_eps + CI + ri, v);
        if (guide) dpm_load<T, V>(eps + (bi + n) * ld_eps + ri, u);
        dpm_load<float, V>(x + i, xv);
        dpm_load<float, V>(noise + i, z);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float e = guide ? step_guide<T>(c[j], u[j], cfg) : c[j];
            const T v1 = (T)(v[j] + 1.0f);
            const float frac = (float)(T)((float)v1 * 0.5f);
            const float rest = (float)(T)(1.0f - frac);
            const float lmax = frac * max_log;
            const float lmin = rest * min_log;
            const float lv = lmax + lmin;
            const float ax = A * xv[j];
            const float be = B * e;
            float p0 = ax - be;
            if (clip) p0 = p0 < -1.0f ? -1.0f : (p0 > 1.0f ? 1.0f : p0);      // a NaN stays one, as torch.clamp leaves it
            x0[j] = p0;
            const float m1 = c1 * p0;
            const float m2 = c2 * xv[j];
            const float mean = m1 + m2;
            const float h = 0.5f * lv;
            const float s = expf(h);
            const float ns = nonzero * s;
            const float nz = ns * z[j];
            out[j] = mean + nz;
        }
        dpm_store<float, V>(xo + i, out);
        if (x0o) dpm_store<float, V>(x0o + i, x0);
        step_store_model<V>(xm, xm_f16, i, total, out);
    }
}

extern "C" int vq_cfg_ddpm_step(const void* eps, const float* x, const float* noise, const float* coef, const int32_t* step,
                                float* x_out, float* x0_out, void* x_model, int n, int C, int inner, long ld_eps, int guided,
                                int row, int n_rows, int eps_f16, int xm_f16, void* stream) {
    const void* const f32[] = {x, noise, x_out, x0_out, nullptr};                 // (x0_out is optional: last)
    int V;
    const int rc = step_check(!x || !noise || !x_out || guided < 0, guided > C, eps, f32, coef, step, x_model, n, C, inner,
                              ld_eps, 2, row, n_rows, eps_f16, xm_f16, &V);
    if (rc != VQ_OK) return rc;
    const long CI = (long)C * inner;
    return step_launch(n, CI, V, eps_f16, [&](auto t, auto v, dim3 grid) {
        typedef decltype(t) T;
        hipLaunchKernelGGL((cfg_ddpm_kernel<T, decltype(v)::value>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)eps,
                           x, noise, coef, step, x_out, x0_out, x_model, xm_f16, n, (long)inner, CI, ld_eps, guided, row,
                           n_rows);
    });
}

// ---- fused CFG + x0 + SA-Solver corrector + next predictor (the PixArt SA-Solver sampling loop) ---------------------
// One launch per model call k of the PEC loop of t2i/diffusion/model/sa_solver.py sample_few_steps (:755-909) as
// sa_sampler.py:75-92 runs it: model_wrapper's guidance (:297-322), data_prediction_fn (:377-386), the corrector
// adams_moulton_update_few_steps (:700-753) of loop step k and the predictor adams_bashforth_update_few_steps (:644-698) of
// loop step k + 1, so the sample the next forward reads leaves the same launch.  Row layout and contract: include/viditq.h
// (vq_cfg_sa_step).  As above nothing is contracted; the guidance is rounded in the model output's type, sigma_t * e is an
// fp32 product (sigma_t is a one-element fp32 tensor in the eager path, which promotes) and the division by alpha_t is the
// correctly rounded fp32 division of a tensor / tensor division.  There is no transcendental.
template <typename T, int V>
__global__ __launch_bounds__(256) void cfg_sa_kernel(const T* __restrict__ eps, const float* x, const float* xp, float* hist,
                                                     const float* __restrict__ noise, const float* __restrict__ coef,
                                                     const int32_t* __restrict__ step, float* xo, float* xpo, void* xm,
                                                     int xm_f16, int n, long CI, long ld_eps, int row, int n_rows) {
#pragma clang fp contract(off)
    const int k = step_row(row, step, n_rows);
    const float* r = coef + (long)k * VQ_SA_ROW;
    const int oc = (int)r[VQ_SA_OC], op = (int)r[VQ_SA_OP];
    const float cfg = r[VQ_SA_CFG], sigma = r[VQ_SA_SIGMA], alpha = r[VQ_SA_ALPHA];
    const float cx = r[VQ_SA_CX], cg0 = r[VQ_SA_CG0], cg1 = r[VQ_SA_CG1], cn = r[VQ_SA_CN];
    const float px = r[VQ_SA_PX], pg0 = r[VQ_SA_PG0], pg1 = r[VQ_SA_PG1], pn = r[VQ_SA_PN];
    const long total = (long)n * CI;
    float* h0 = hist + (long)(k % 2) * total;                    // written: m_k
    const float* h1 = hist + (long)((k + 1) % 2) * total;        // m_{k-1}
    const float* z0 = noise + (long)(k % 2) * total;             // the draw of loop step k (corrector)
    const float* z1 = noise + (long)((k + 1) % 2) * total;       // the draw of loop step k + 1 (predictor)
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * V; i < total; i += (long)gridDim.x * blockDim.x * V) {
        const long bi = i / CI, ri = i - bi * CI;
        float u[V], c[V], xv[V], pv[V], m1[V], zc[V], zp[V], m0[V], xc[V], xq[V];
        dpm_load<T, V>(eps + bi * ld_eps + ri, u);
        dpm_load<T, V>(eps + (bi + n) * ld_eps + ri, c);
        dpm_load<float, V>(x + i, xv);
        dpm_load<float, V>(xp + i, pv);
        if (oc == 2 || op == 2) dpm_load<float, V>(h1 + i, m1);
        if (oc >= 1) dpm_load<float, V>(z0 + i, zc);
        if (op >= 1) dpm_load<float, V>(z1 + i, zp);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float e = step_guide<T>(c[j], u[j], cfg);
            const float se = sigma * e;
            const float t = pv[j] - se;
            const float m = __fdiv_rn(t, alpha);
            m0[j] = m;
            float v = xv[j];
            if (oc >= 1) {
                float g = cg0 * m;
                if (oc == 2) {
                    const float g1 = cg1 * m1[j];
                    g = g + g1;
                }
                const float a = cx * v;
                const float ag = a + g;
                const float nz = cn * zc[j];
                v = ag + nz;
            }
            xc[j] = v;
            if (op >= 1) {
                float q = pg0 * m;
                if (op == 2) {
                    const float q1 = pg1 * m1[j];
                    q = q + q1;
                }
                const float a = px * v;
                const float aq = a + q;
                const float nz = pn * zp[j];
                v = aq + nz;
            }
            xq[j] = v;
        }
        dpm_store<float, V>(h0 + i, m0);
        dpm_store<float, V>(xo + i, xc);
        dpm_store<float, V>(xpo + i, xq);
        step_store_model<V>(xm, xm_f16, i, total, xq);
    }
}

extern "C" int vq_cfg_sa_step(const void* eps, const float* x, const float* xp, float* hist, const float* noise,
                              const float* coef, const int32_t* step, float* x_out, float* xp_out, void* x_model, int n, int C,
                              int inner, long ld_eps, int row, int n_rows, int eps_f16, int xm_f16, void* stream) {
    const void* const f32[] = {x, xp, hist, noise, x_out, xp_out, nullptr};
    int V;
    const int rc = step_check(!x || !xp || !hist || !noise || !x_out || !xp_out, false, eps, f32, coef, step, x_model, n, C,
                              inner, ld_eps, 1, row, n_rows, eps_f16, xm_f16, &V);
    if (rc != VQ_OK) return rc;
    const long CI = (long)C * inner;
    return step_launch(n, CI, V, eps_f16, [&](auto t, auto v, dim3 grid) {
        typedef decltype(t) T;
        hipLaunchKernelGGL((cfg_sa_kernel<T, decltype(v)::value>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)eps, x,
                           xp, hist, noise, coef, step, x_out, xp_out, x_model, xm_f16, n, CI, ld_eps, row, n_rows);
    });
}
