// K0, the ELU(1) object (psnode_generic_impl.h), and the host's plan / fit / pack code, which every build shares and which is compiled here once.
#define PSNODE_BUILD BuildElu1
#include "psnode_generic_impl.h"

namespace psnode {

namespace {
struct PackArgs {
    int n;                       // layers in total (de then ae)
    int xd, nall, nzv;           // state dims, width of all_initial, z + v dims: the column orders of the two first layers
    int perm[2 * kMaxLayers];    // 0: columns as they are, 1: DE first layer (de_orig_col), 2: AE first layer (ae_orig_col),
                                 // 3: the TRANSPOSED matrix (tiles over the layer's inputs, contraction over its outputs; no bias)
    int K[2 * kMaxLayers], N[2 * kMaxLayers];
    const float* w[2 * kMaxLayers];
    const float* b[2 * kMaxLayers];
    float* img[2 * kMaxLayers];
};

// The MFMA image of every layer of both MLPs in one launch (blockIdx.y = layer): [tile nt][q][lane] f4, component c = W[16 nt + lane % 16]
// [16 q + 4 (lane / 16) + c] (zero outside the matrix), then the bias padded to 16 * tiles.
__global__ void pack_image_kernel(const PackArgs p) {
    const int l = blockIdx.y;
    const int K = p.K[l], N = p.N[l], perm = p.perm[l];
    if (perm == 3) {             // image of W^T: rows j < K, contraction kn < N
        const int S4 = (N + 15) >> 4, NTL = (K + 15) >> 4;
        const float* __restrict__ w = p.w[l];
        float* __restrict__ img = p.img[l];
        const int nw = NTL * S4 * 256;
        for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < nw + 16 * NTL; idx += gridDim.x * blockDim.x) {
            if (idx >= nw) { img[idx] = 0.0f; continue; }
            const int c = idx & 3, lane = (idx >> 2) & 63, q = (idx >> 8) % S4, nt = (idx >> 8) / S4;
            const int j = 16 * nt + (lane & 15), kn = 16 * q + 4 * (lane >> 4) + c;
            img[idx] = (j < K && kn < N) ? w[(size_t)kn * K + j] : 0.0f;
        }
        return;
    }
    const int K16 = perm == 1 ? de_k16(p.xd, p.nall) : (perm == 2 ? ae_k16(p.xd, p.nzv, p.nall) : up16(K));
    const int S4 = K16 >> 4, NTL = (N + 15) >> 4;
    const float* __restrict__ w = p.w[l];
    float* __restrict__ img = p.img[l];
    const int nw = NTL * S4 * 256;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < nw + 16 * NTL; idx += gridDim.x * blockDim.x) {
        if (idx >= nw) { const int j = idx - nw; img[idx] = j < N ? p.b[l][j] : 0.0f; continue; }
        const int c = idx & 3, lane = (idx >> 2) & 63, q = (idx >> 8) % S4, nt = (idx >> 8) / S4;
        const int j = 16 * nt + (lane & 15), kn = 16 * q + 4 * (lane >> 4) + c;
        const int k = perm == 1 ? de_orig_col(kn, p.xd, p.nall) : (perm == 2 ? ae_orig_col(kn, p.xd, p.nzv, p.nall) : (kn < K ? kn : -1));
        img[idx] = (j < N && k >= 0) ? w[(size_t)j * K + k] : 0.0f;
    }
}

void add_pack(PackArgs& p, const MlpDev& d, int perm0) {
    int k = d.in_dim;
    for (int l = 0; l < d.n_layers; ++l) {
        p.perm[p.n] = l ? 0 : perm0;
        p.K[p.n] = k;
        p.N[p.n] = d.out_dim[l];
        p.w[p.n] = d.w[l];
        p.b[p.n] = d.bias[l];
        p.img[p.n] = const_cast<float*>(d.wt[l]);
        ++p.n;
        k = d.out_dim[l];
    }
}

struct PackTArgs {
    int n;
    int K[2 * kMaxLayers], N[2 * kMaxLayers];
    const float* w[2 * kMaxLayers];
    float* wt[2 * kMaxLayers];
};

// wt[k][j] = w[j][k] for every layer of both MLPs in one launch (blockIdx.y = layer): the generic BACKWARD's weight layout.
__global__ void pack_transpose_kernel(const PackTArgs p) {
    const int l = blockIdx.y;
    const int K = p.K[l], N = p.N[l];
    const float* __restrict__ w = p.w[l];
    float* __restrict__ wt = p.wt[l];
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < K * N; idx += gridDim.x * blockDim.x) {
        const int k = idx / N, j = idx % N;
        wt[idx] = w[(size_t)j * K + k];
    }
}

void add_pack_t(PackTArgs& p, const MlpDev& d) {
    int k = d.in_dim;
    for (int l = 0; l < d.n_layers; ++l) {
        p.K[p.n] = k;
        p.N[p.n] = d.out_dim[l];
        p.w[p.n] = d.w[l];
        p.wt[p.n] = const_cast<float*>(d.wt[l]);
        ++p.n;
        k = d.out_dim[l];
    }
}

}  // namespace

// wt[k][j] = w[j][k] for every layer of one or two MLPs, one launch (generic backward)
hipError_t launch_pack_transpose(const MlpDev& de, const MlpDev* ae, hipStream_t stream) {
    PackTArgs p;
    p.n = 0;
    add_pack_t(p, de);
    if (ae) add_pack_t(p, *ae);
    hipLaunchKernelGGL(pack_transpose_kernel, dim3(8, p.n), dim3(256), 0, stream, p);
    return hipGetLastError();
}

// Plain (natural column order, with bias) and transposed images of one MLP's layers for the generic backward's register path: img[l] /
// imgT[l] must hold generic_image_floats(K_l, N_l) / generic_image_floats(N_l, K_l) floats.
hipError_t launch_pack_plain_images(const MlpDev& m, float* const* img, float* const* imgT, hipStream_t stream) {
    PackArgs p;
    p.n = 0; p.xd = 0; p.nall = 0; p.nzv = 0;
    int k = m.in_dim;
    for (int l = 0; l < m.n_layers; ++l) {
        for (int t = 0; t < 2; ++t) {
            p.perm[p.n] = t ? 3 : 0;
            p.K[p.n] = k; p.N[p.n] = m.out_dim[l];
            p.w[p.n] = m.w[l]; p.b[p.n] = m.bias[l];
            p.img[p.n] = t ? imgT[l] : img[l];
            ++p.n;
        }
        k = m.out_dim[l];
    }
    hipLaunchKernelGGL(pack_image_kernel, dim3(16, p.n), dim3(256), 0, stream, p);
    return hipGetLastError();
}

// floats of the generic forward's workspace segment of one layer (psnode_capi.hip: bind_mlp takes one per layer)
size_t generic_image_floats(int K, int N) { return image_floats(K, N); }

// the MFMA images of one or two MLPs (d.wt[l] = the layer's segment, generic_image_floats each), one launch
hipError_t launch_pack_image(const MlpDev& de, const MlpDev* ae, int xd, int n, int nzv, hipStream_t stream) {
    PackArgs p;
    p.n = 0;
    p.xd = xd; p.nall = n; p.nzv = nzv;
    add_pack(p, de, 1);
    if (ae) add_pack(p, *ae, 2);
    hipLaunchKernelGGL(pack_image_kernel, dim3(16, p.n), dim3(256), 0, stream, p);
    return hipGetLastError();
}

// LDS of the kernel without any resident image: activations, state, biases
size_t generic_lds_bytes(const IntegrateDev& a, bool dae, int lin) {
    const int vd = dae ? a.vd : 0, id = dae ? a.id : 0;
    const int n = a.xd + a.zd + vd + id;
    const int nzv = a.zd + vd;
    // DE input, AE input, two layer-output buffers, a0, ext, xcur + xsrc, kbuf, icur, zvn, dts; lin 1: the interval's left z | v rows, 2: the four node rows of the Lagrange stencil
    const size_t rows = (size_t)de_k16(a.xd, n) + (dae ? ae_k16(a.xd, nzv, n) : 0) + 2 * (size_t)up16(a.maxo) + n + (n - a.xd) + 2 * (size_t)a.xd +
                        4 * (size_t)a.xd + id + nzv + 1 + (lin == 2 ? 4 * nzv : (lin ? nzv : 0));
    return (rows * TB + generic_bias_floats(a, dae)) * sizeof(float);
}

// Which layers' images become resident: greedy in layer order, DE (evaluated once per stage) before AE (once per step).  Returns the
// launch's LDS bytes; `mask`: bit l = DE layer l, bit 8 + l = AE layer l.
// Register mode (mlp_reg): layers of at most four tiles (one per wave), the first layers' LEADING blocks (DE: 2 x_dim columns, AE: x | z | v)
// within 16 * QM columns -- the rest of a first layer is folded (fold0), so z / v / i may be as wide as LDS holds; at most four layers per
// MLP for the DAE (two MLPs: 160 operand registers at QM 8), eight for the ODE (144).  Returns QM (4 or 8), or 0.
int generic_reg_mode(const IntegrateDev& a, bool dae) {
    // the leading blocks of the two first layers (state columns / x | z | v): what the registers hold of layer 0
    const int lead_de = de_sx(a.xd), lead_ae = dae ? ae_sa(a.xd, a.zd + a.vd) : 0;
    if (lead_de > 128 || lead_ae > 128) return 0;
    for (int m = 0; m < (dae ? 2 : 1); ++m) {
        const MlpDev& d = m ? a.ae : a.de;
        if (d.n_layers > (dae ? 4 : kMaxLayers)) return 0;
        for (int l = 0; l < d.n_layers; ++l)
            if (d.out_dim[l] > 64) return 0;
    }
    return (lead_de <= 64 && lead_ae <= 64) ? 4 : 8;
}

// Wide register form (mlp_regw; ODE): 2 .. 4 layers, hidden layers within 128 units, every contraction within 128 columns, at most 64 outputs
bool generic_wide_mode(const IntegrateDev& a, bool dae) {
    if (dae || a.de.n_layers < 2 || a.de.n_layers > 4 || de_sx(a.xd) > 128) return false;
    for (int l = 0; l < a.de.n_layers; ++l)
        if (a.de.out_dim[l] > (l + 1 == a.de.n_layers ? 64 : 128)) return false;
    return true;
}

size_t generic_plan(const IntegrateDev& a, bool dae, unsigned& mask, int lin) {
    size_t bytes = generic_lds_bytes(a, dae, lin);
    mask = 0;
    if (generic_reg_mode(a, dae) || generic_wide_mode(a, dae)) return bytes;
    const size_t limit = 160 * 1024;
    for (int m = 0; m < (dae ? 2 : 1); ++m) {
        const MlpDev& d = m ? a.ae : a.de;
        const int vd_ = dae ? a.vd : 0, n_ = a.xd + a.zd + vd_ + (dae ? a.id : 0);
        int K = m ? ae_k16(a.xd, a.zd + vd_, n_) : de_k16(a.xd, n_);
        for (int l = 0; l < d.n_layers; ++l) {
            const size_t img = (size_t)up16(d.out_dim[l]) * up16(K) * sizeof(float);
            if (bytes + img <= limit) { bytes += img; mask |= 1u << (8 * m + l); }
            K = d.out_dim[l];
        }
    }
    return bytes;
}

}  // namespace psnode
