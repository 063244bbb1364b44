// rtw_denoise.hip -- the preview denoiser of rtw.h (rtw_denoiser_*, rtw_denoise_host).
//
// The arithmetic is include/rtw_denoise.h's, one text for the kernels here, the host twin and the stand-alone
// check program.  Three small kernels, nothing persistent: one pixel per lane, 256-thread blocks over patches of
// 64 x 4 pixels, so that a wave's 64 lanes read 1 KiB of contiguous 16-byte records per tap.  The levels
// ping-pong between the denoiser's two record buffers; the last level writes the interleaved image (and the
// variance) itself.
#include <cstdlib>
#include <string>
#include <utility>

#include <hip/hip_runtime.h>

#include "rtw_common.h"
#include "../../include/rtw_denoise.h"

#define RTW_DENOISE_BX 64
#define RTW_DENOISE_BY 4

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess)                                                                     \
            return rtw::fail(RTW_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));    \
    } while (0)

// the lane's pixel; false for the lanes past the right and bottom edges
__device__ inline bool denoise_lane_pixel(int W, int H, int* x, int* y) {
    *x = (int)blockIdx.x * RTW_DENOISE_BX + ((int)threadIdx.x & (RTW_DENOISE_BX - 1));
    *y = (int)blockIdx.y * RTW_DENOISE_BY + ((int)threadIdx.x / RTW_DENOISE_BX);
    return *x < W && *y < H;
}

// inputs -> the level-0 records and the padded guides (reads nothing but the inputs, writes nothing but scratch)
__global__ __launch_bounds__(RTW_DENOISE_BX* RTW_DENOISE_BY) void denoise_prep_kernel(
    const float* __restrict__ color, const float* __restrict__ std_err, const float* __restrict__ guide, int gc, int W,
    int H, rtw_denoise_rec* __restrict__ rec, rtw_denoise_rec* __restrict__ guide4) {
    int x, y;
    if (!denoise_lane_pixel(W, H, &x, &y)) return;
    const size_t at = (size_t)y * (size_t)W + (size_t)x;
    rec[at] = rtw_denoise_prep_pixel(color, std_err, guide, gc, W, H, x, y);
    if (gc > 0) guide4[at] = rtw_denoise_guide_pixel(guide, gc, at);
}

// one level: src -> dst, or with LAST -> the image and, when asked, the variance
template <bool GUIDE, bool LAST>
__global__ __launch_bounds__(RTW_DENOISE_BX* RTW_DENOISE_BY) void denoise_level_kernel(
    const rtw_denoise_rec* __restrict__ src, const rtw_denoise_rec* __restrict__ guide4, int W, int H, int step,
    float sigma_l, float inv_sg2, rtw_denoise_rec* __restrict__ dst, float* __restrict__ out,
    float* __restrict__ out_variance) {
    int x, y;
    if (!denoise_lane_pixel(W, H, &x, &y)) return;
    const size_t at = (size_t)y * (size_t)W + (size_t)x;
    // (the padded guide channels are zeros: 4 channels give the bits of guide_channels channels, rtw_denoise.h)
    const rtw_denoise_rec o = rtw_denoise_level_pixel(src, guide4, GUIDE ? 4 : 0, W, H, x, y, step, sigma_l, inv_sg2);
    if (LAST) {
        out[3 * at] = o.r;
        out[3 * at + 1] = o.g;
        out[3 * at + 2] = o.b;
        if (out_variance) out_variance[at] = o.w;
    } else {
        dst[at] = o;
    }
}

// the same with an albedo image (rtw_denoiser_run_albedo): prep on the demodulated inputs ...
__global__ __launch_bounds__(RTW_DENOISE_BX* RTW_DENOISE_BY) void denoise_prep_albedo_kernel(
    const float* __restrict__ color, const float* __restrict__ std_err, const float* __restrict__ guide,
    const float* __restrict__ albedo, int gc, int W, int H, rtw_denoise_rec* __restrict__ rec,
    rtw_denoise_rec* __restrict__ guide4) {
    int x, y;
    if (!denoise_lane_pixel(W, H, &x, &y)) return;
    const size_t at = (size_t)y * (size_t)W + (size_t)x;
    rec[at] = rtw_denoise_prep_pixel_albedo(color, std_err, guide, albedo, gc, W, H, x, y);
    if (gc > 0) guide4[at] = rtw_denoise_guide_pixel(guide, gc, at);
}

// ... and the last level, which multiplies the albedo back in, or hands a pixel that was left out its input colour.
// `out` may be `color` (hence no __restrict__ on the two): a lane reads its own pixel's inputs, then writes it.
template <bool GUIDE>
__global__ __launch_bounds__(RTW_DENOISE_BX* RTW_DENOISE_BY) void denoise_level_albedo_kernel(
    const rtw_denoise_rec* __restrict__ src, const rtw_denoise_rec* __restrict__ guide4, const float* color,
    const float* __restrict__ albedo, int W, int H, int step, float sigma_l, float inv_sg2, float* out,
    float* __restrict__ out_variance) {
    int x, y;
    if (!denoise_lane_pixel(W, H, &x, &y)) return;
    const size_t at = (size_t)y * (size_t)W + (size_t)x;
    const rtw_denoise_rec f = rtw_denoise_level_pixel(src, guide4, GUIDE ? 4 : 0, W, H, x, y, step, sigma_l, inv_sg2);
    float o[3];
    rtw_denoise_remodulate(color, albedo, at, f, o);
    out[3 * at] = o[0];
    out[3 * at + 1] = o[1];
    out[3 * at + 2] = o[2];
    if (out_variance) out_variance[at] = f.w;
}

struct rtw_denoiser {
    int device = 0;
    int32_t width = 0, height = 0;
    rtw_denoise_rec* scratch = nullptr;  // RTW_DENOISE_SCRATCH_RECS * width * height records
};

namespace {

int check_params(const rtw_denoise_params* p) {
    if (!p) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null params");
    const char* field = rtw_denoise_check(p);
    if (field) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, std::string("rtw_denoise_params.") + field + " is out of range");
    return RTW_OK;
}

template <bool GUIDE, bool LAST>
void launch_level(dim3 grid, hipStream_t stream, const rtw_denoise_rec* src, const rtw_denoise_rec* guide4,
                  const rtw_denoise_params& p, int step, float inv_sg2, rtw_denoise_rec* dst, float* out,
                  float* out_variance) {
    hipLaunchKernelGGL((denoise_level_kernel<GUIDE, LAST>), grid, dim3(RTW_DENOISE_BX * RTW_DENOISE_BY), 0, stream, src,
                       guide4, p.width, p.height, step, p.sigma_l, inv_sg2, dst, out, out_variance);
}

}  // namespace

extern "C" RTW_API int rtw_denoiser_create(int device, int32_t width, int32_t height, rtw_denoiser** out) {
    if (!out) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    if (width < 2) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "width must be >= 2");
    if (height < 2) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "height must be >= 2");
    // (the grid of 64 x 4 patches stays inside HIP's 2^31 - 1 threads per dimension)
    if (width > (1 << 24) || height > (1 << 24)) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "width and height must be <= 2^24");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return rtw::fail(RTW_ERR_NO_DEVICE, "no HIP device: the MI355X path requires a GPU (there is no CPU fallback)");
    if (device < 0 || device >= ndev) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    const size_t bytes = (size_t)RTW_DENOISE_SCRATCH_RECS * (size_t)width * (size_t)height * sizeof(rtw_denoise_rec);
    rtw_denoise_rec* scratch = nullptr;
    if (hipMalloc(&scratch, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return rtw::fail(RTW_ERR_OUT_OF_MEMORY, "no device memory for the denoiser's scratch");
    }
    auto* d = new rtw_denoiser;
    d->device = device;
    d->width = width;
    d->height = height;
    d->scratch = scratch;
    *out = d;
    return RTW_OK;
}

extern "C" RTW_API int rtw_denoiser_release(rtw_denoiser* d) {
    if (!d) return RTW_OK;
    (void)hipSetDevice(d->device);
    (void)hipFree(d->scratch);  // (waits for the runs that still read it)
    delete d;
    return RTW_OK;
}

extern "C" RTW_API int rtw_denoiser_run_albedo(rtw_denoiser* d, const rtw_denoise_params* params, const float* d_color,
                                               const float* d_stderr, const float* d_guide, const float* d_albedo,
                                               float* d_out, float* d_out_variance, void* stream_) {
    if (!d) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null denoiser");
    const int v = check_params(params);
    if (v != RTW_OK) return v;
    const rtw_denoise_params& p = *params;
    if (p.width != d->width) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "rtw_denoise_params.width is not the denoiser's");
    if (p.height != d->height) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "rtw_denoise_params.height is not the denoiser's");
    if (!d_color) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null d_color");
    if (!d_stderr) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null d_stderr");
    if (!d_guide && p.guide_channels > 0) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null d_guide with guide_channels > 0");
    if (!d_out) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null d_out");
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(d->device));
    const size_t n = (size_t)p.width * (size_t)p.height;
    rtw_denoise_rec* src = d->scratch;
    rtw_denoise_rec* dst = d->scratch + n;
    rtw_denoise_rec* guide4 = d->scratch + 2 * n;
    const dim3 grid((unsigned)((p.width + RTW_DENOISE_BX - 1) / RTW_DENOISE_BX),
                    (unsigned)((p.height + RTW_DENOISE_BY - 1) / RTW_DENOISE_BY));
    const bool guided = p.guide_channels > 0;
    const float inv_sg2 = rtw_denoise_inv_sg2(p.sigma_g);
    if (d_albedo)
        hipLaunchKernelGGL(denoise_prep_albedo_kernel, grid, dim3(RTW_DENOISE_BX * RTW_DENOISE_BY), 0, stream, d_color,
                           d_stderr, d_guide, d_albedo, (int)p.guide_channels, (int)p.width, (int)p.height, src, guide4);
    else
        hipLaunchKernelGGL(denoise_prep_kernel, grid, dim3(RTW_DENOISE_BX * RTW_DENOISE_BY), 0, stream, d_color, d_stderr,
                           d_guide, (int)p.guide_channels, (int)p.width, (int)p.height, src, guide4);
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < p.iterations; ++i) {
        const int step = 1 << i;
        if (i + 1 < p.iterations) {
            if (guided)
                launch_level<true, false>(grid, stream, src, guide4, p, step, inv_sg2, dst, nullptr, nullptr);
            else
                launch_level<false, false>(grid, stream, src, guide4, p, step, inv_sg2, dst, nullptr, nullptr);
            std::swap(src, dst);
        } else if (d_albedo) {
            if (guided)
                hipLaunchKernelGGL((denoise_level_albedo_kernel<true>), grid, dim3(RTW_DENOISE_BX * RTW_DENOISE_BY), 0, stream,
                                   (const rtw_denoise_rec*)src, (const rtw_denoise_rec*)guide4, d_color, d_albedo,
                                   (int)p.width, (int)p.height, step, p.sigma_l, inv_sg2, d_out, d_out_variance);
            else
                hipLaunchKernelGGL((denoise_level_albedo_kernel<false>), grid, dim3(RTW_DENOISE_BX * RTW_DENOISE_BY), 0, stream,
                                   (const rtw_denoise_rec*)src, (const rtw_denoise_rec*)guide4, d_color, d_albedo,
                                   (int)p.width, (int)p.height, step, p.sigma_l, inv_sg2, d_out, d_out_variance);
        } else if (guided) {
            launch_level<true, true>(grid, stream, src, guide4, p, step, inv_sg2, nullptr, d_out, d_out_variance);
        } else {
            launch_level<false, true>(grid, stream, src, guide4, p, step, inv_sg2, nullptr, d_out, d_out_variance);
        }
        HIP_TRY(hipGetLastError());
    }
    return RTW_OK;
}

extern "C" RTW_API int rtw_denoiser_run(rtw_denoiser* d, const rtw_denoise_params* params, const float* d_color,
                                        const float* d_stderr, const float* d_guide, float* d_out, float* d_out_variance,
                                        void* stream) {
    return rtw_denoiser_run_albedo(d, params, d_color, d_stderr, d_guide, nullptr, d_out, d_out_variance, stream);
}

extern "C" RTW_API int rtw_denoise_host_albedo(const rtw_denoise_params* params, const float* color, const float* std_err,
                                               const float* guide, const float* albedo, float* out, float* out_variance) {
    const int v = check_params(params);
    if (v != RTW_OK) return v;
    if (!color) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null color");
    if (!std_err) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null std_err");
    if (!guide && params->guide_channels > 0) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null guide with guide_channels > 0");
    if (!out) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null out");
    const size_t n = (size_t)params->width * (size_t)params->height;
    auto* scratch = (rtw_denoise_rec*)std::aligned_alloc(16, RTW_DENOISE_SCRATCH_RECS * n * sizeof(rtw_denoise_rec));
    if (!scratch) return rtw::fail(RTW_ERR_OUT_OF_MEMORY, "no host memory for the denoiser's scratch");
    const int rc = rtw_denoise_image_albedo(params, color, std_err, guide, albedo, out, out_variance, scratch);
    std::free(scratch);
    return rc == 0 ? RTW_OK : rtw::fail(RTW_ERR_INVALID_ARGUMENT, "bad rtw_denoise_params");
}

extern "C" RTW_API int rtw_denoise_host(const rtw_denoise_params* params, const float* color, const float* std_err,
                                        const float* guide, float* out, float* out_variance) {
    return rtw_denoise_host_albedo(params, color, std_err, guide, nullptr, out, out_variance);
}
