// The losses of the watermark training step, one kernel per direction, and the opening kernel of a captured step.
//
// On this path a "tensor" is a few thousand rays, so every stock elementwise/reduction operator is a ~3 us launch and the
// reference's op chains (renderer_wtmk.py:316-319: background mix and depth normalisation, csrc/composite.hip; utils_wtmk_disen.py:615-640:
// MSE + BCE-with-logits + weighted sum, and their autograd backward) come to ~60 launches per step: 0.2 ms of a 1.8 ms step.
#include "wave.h"

namespace nsig {

// loss_i = mean((content - gt)^2); loss_w = mean BCE-with-logits(temp * decoded, message); loss = lambda_w*loss_w + lambda_i*loss_i.
// One workgroup; also leaves the two gradient directions d(loss_i)/d(content), d(loss_w)/d(decoded) for the backward kernel.
__global__ void __launch_bounds__(1024) k_wm_loss_fwd(const float *__restrict__ content, const float *__restrict__ gt, uint32_t n_content,
                                                      const float *__restrict__ decoded, const float *__restrict__ message, uint32_t D, float temp,
                                                      float lambda_w, float lambda_i, float *__restrict__ losses, float *__restrict__ d_content,
                                                      float *__restrict__ d_decoded) {
    __shared__ float scratch[16];
    float si = 0.0f, sw = 0.0f;
    const float ki = 2.0f / (float)n_content, kw = temp / (float)D;
    for (uint32_t i = threadIdx.x; i < n_content; i += 1024) {
        const float d = content[i] - gt[i];
        si += d * d;
        d_content[i] = ki * d;
    }
    for (uint32_t i = threadIdx.x; i < D; i += 1024) {
        const float x = temp * decoded[i], y = message[i];
        // binary_cross_entropy_with_logits: (1 - y) * x + log(1 + exp(-|x|)) + max(-x, 0)
        sw += (1.0f - y) * x + fmaxf(-x, 0.0f) + log1pf(expf(-fabsf(x)));
        d_decoded[i] = kw * (1.0f / (1.0f + expf(-x)) - y);
    }
    si = block_sum(si, scratch);
    sw = block_sum(sw, scratch);
    if (threadIdx.x == 0) {
        const float li = si / (float)n_content, lw = sw / (float)D;
        losses[0] = li;
        losses[1] = lw;
        losses[2] = lambda_w * lw + lambda_i * li;
    }
}

// grads: [g_lossi, g_lossw, g_loss] (device scalars; a null pointer is 0).
__global__ void __launch_bounds__(256) k_wm_loss_bwd(const float *__restrict__ g_li, const float *__restrict__ g_lw, const float *__restrict__ g_l,
                                                     float lambda_w, float lambda_i, const float *__restrict__ d_content, uint32_t n_content,
                                                     const float *__restrict__ d_decoded, uint32_t D, float *__restrict__ g_content,
                                                     float *__restrict__ g_decoded) {
    const float gl = g_l ? g_l[0] : 0.0f;
    const float ci = (g_li ? g_li[0] : 0.0f) + lambda_i * gl, cw = (g_lw ? g_lw[0] : 0.0f) + lambda_w * gl;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_content) g_content[i] = ci * d_content[i];
    if (i < D) g_decoded[i] = cw * d_decoded[i];
}

// Opening kernel of a captured training step: zero-fills the shared gradient buffer (torch's zero_grad) and stages this
// step's message words from a ring in pinned host memory into the device tensor the step's kernels read -- slot = the number
// of replays so far modulo `slots`, counted on the device, so a replayed graph needs no host-to-device copy in front of it.
__global__ void __launch_bounds__(256) k_step_begin(float4 *__restrict__ G4, uint32_t n4, const float *__restrict__ ring, uint32_t slots, uint32_t width,
                                                    uint32_t *__restrict__ counter, float *__restrict__ msg) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n4) G4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (blockIdx.x == 0) {
        const uint32_t slot = *counter % slots;      // every thread reads the count before thread 0 advances it
        if (threadIdx.x < width) msg[threadIdx.x] = ring[(size_t)slot * width + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0) *counter = *counter + 1u;
    }
}

}  // namespace nsig

using namespace nsig;

NSIG_EXPORT void *nsig_host_device_pointer(const void *pinned_host) {
    void *dev = nullptr;
    if (pinned_host == nullptr || hipHostGetDevicePointer(&dev, const_cast<void *>(pinned_host), 0) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return dev;
}

NSIG_EXPORT int loop_step_begin(float *G, uint32_t n_floats, const float *ring_dev, uint32_t slots, uint32_t width, uint32_t *counter, float *msg,
                                nsig_stream_t stream) {
    NSIG_REQUIRE(G && ring_dev && counter && msg, "loop_step_begin: null pointer");
    NSIG_REQUIRE(aligned16(G) && n_floats % 4 == 0, "loop_step_begin: G must be 16-byte aligned with a multiple of 4 floats");
    NSIG_REQUIRE(slots >= 1 && width >= 1 && width <= 256, "loop_step_begin: slots >= 1 and 1 <= width <= 256");
    const uint32_t n4 = n_floats / 4;
    k_step_begin<<<ceil_div(n4 > 0 ? n4 : 1u, 256u), 256, 0, as_stream(stream)>>>(reinterpret_cast<float4 *>(G), n4, ring_dev, slots,
                                                                                 width, counter, msg);
    return check_launch("loop_step_begin");
}

NSIG_EXPORT int wm_loss_fwd(const float *content, const float *gt, uint32_t n_content, const float *decoded, const float *message, uint32_t D,
                            float temp, float lambda_w, float lambda_i, float *losses3, float *d_content, float *d_decoded, nsig_stream_t stream) {
    NSIG_REQUIRE(content && gt && decoded && message && losses3 && d_content && d_decoded, "wm_loss_fwd: null pointer");
    NSIG_REQUIRE(n_content >= 1 && D >= 1, "wm_loss_fwd: empty input");
    k_wm_loss_fwd<<<1, 1024, 0, as_stream(stream)>>>(content, gt, n_content, decoded, message, D, temp, lambda_w, lambda_i, losses3, d_content, d_decoded);
    return check_launch("wm_loss_fwd");
}

NSIG_EXPORT int wm_loss_bwd(const float *g_lossi, const float *g_lossw, const float *g_loss, float lambda_w, float lambda_i, const float *d_content,
                            uint32_t n_content, const float *d_decoded, uint32_t D, float *grad_content, float *grad_decoded, nsig_stream_t stream) {
    NSIG_REQUIRE(d_content && d_decoded && grad_content && grad_decoded, "wm_loss_bwd: null pointer");
    const uint32_t n = n_content > D ? n_content : D;
    k_wm_loss_bwd<<<ceil_div(n, 256u), 256, 0, as_stream(stream)>>>(g_lossi, g_lossw, g_loss, lambda_w, lambda_i, d_content, n_content, d_decoded, D,
                                                                    grad_content, grad_decoded);
    return check_launch("wm_loss_bwd");
}
