/*
 * psnode_hip.h -- C ABI of the MI355X (gfx950) fixed-grid neural-ODE/DAE integrator.
 *
 * This is the drop-in boundary for the hot path of xxh0523/Py_PSNODE.  The reference has no FFI of
 * its own (it is pure Python/PyTorch); each entry point below replaces the
 * Python interface named in its comment (file:line under /root/reference), and is what a ctypes
 * binding inside the reference's `neural_dae` package would bind (INTEGRATION.md shows that stub).
 *
 * Conventions
 *   - plain C: pointers, sizes, POD structs.  No torch types.  All float data is fp32.
 *   - every pointer is a DEVICE pointer unless the comment says "host".
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t passed as void*); no call
 *     synchronises the device, allocates user-visible memory or keeps a reference to its arguments
 *     beyond the enqueue.  Re-entrant across streams/devices; no global mutable state.
 *   - scratch memory is caller-provided (`workspace`); its size comes from psnode_workspace_bytes().
 *   - return value: PSNODE_OK (0) or a negative psnode_status; never throws/aborts.
 *     psnode_status_string() maps a status to text.
 *   - tensors are TIME-MAJOR logical [T,B,D] views described by (ptr, stride_t, stride_b) in ELEMENTS
 *     with the last dimension contiguous -- exactly what the scripts hand the solver:
 *     `x.permute(1,0,2)` of B-major [B,T,D] memory (neural_00_ODE_01_no_encode.py:82-84).
 */
#ifndef PSNODE_HIP_H
#define PSNODE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSNODE_ABI_VERSION 10    /* 10 also carries the additive psnode_act_f32 / *_act_*, psnode_rk_tableau_f32 / *_rk_*, psnode_substeps_f32 / *_sub_*, *_lin_*, *_pev_* / psnode_event_table_pt_f32, *_ab_*, *_ab3_*, *_lag_* / psnode_ext_stencil_f32 and psnode_dae_*_sth_* entry points (end of this file), and psnode_loss_fn_f32 / psnode_masked_loss_* / psnode_loss_per_sample_f32 (next to psnode_masked_mse_f32) */
#define PSNODE_MAX_LAYERS 8      /* Linear layers per MLP */
#define PSNODE_MAX_WIDTH 1024    /* widest layer OUTPUT the kernels accept */
#define PSNODE_MAX_IN_WIDTH 2048 /* widest first-layer INPUT (the latent DE of DAE_02 at --hidden 128 is 12 x 128 = 1536 wide) */

typedef enum {
    PSNODE_OK = 0,
    PSNODE_ERR_NULL = -1,        /* required pointer is NULL */
    PSNODE_ERR_DIMS = -2,        /* bad / inconsistent dimensions (e.g. first Linear in_features != recipe) */
    PSNODE_ERR_METHOD = -3,      /* unknown method id */
    PSNODE_ERR_WORKSPACE = -4,   /* workspace too small or misaligned */
    PSNODE_ERR_UNSUPPORTED = -5, /* shape outside kernel limits, or the requested kernel is not available for it */
    PSNODE_ERR_HIP = -6          /* a HIP runtime call failed (launch error, bad stream, ...) */
} psnode_status;

/* my_fixed_grid.py:12 (Euler), :20 (Midpoint), :35 (RK4 = 3/8-rule rk4_alt_step_func) */
typedef enum { PSNODE_EULER = 0, PSNODE_MIDPOINT = 1, PSNODE_RK4_38 = 2 } psnode_method;

/* kernel selection: AUTO picks the MFMA kernel when the shape has one, else the generic kernel */
typedef enum {
    PSNODE_KERNEL_AUTO = 0, PSNODE_KERNEL_GENERIC = 1, PSNODE_KERNEL_MFMA = 2,
    PSNODE_KERNEL_MFMA_TILE = 4,     /* K1 / K2, the 4-waves-per-16-trajectory-tile MFMA integrators, where AUTO / MFMA would pick K1x / K2x; psnode_ode_backward_f32: K4f */
    PSNODE_KERNEL_MFMA_WAVE = 5,     /* K1x / K2x, the one-wave-per-4-trajectories (exchange-free) MFMA integrators (incl. their saving instances);
                                        psnode_ode_backward_f32: K4x, the backward of the same form (hidden 33..64, saved rows); UNSUPPORTED outside their shapes */
    PSNODE_KERNEL_MFMA_WIDE = 3      /* backward calls only: the one-launch MFMA backward K4f (hidden <= 128 zero-padded to 32 / 64 / 128); since ABI 8
                                        (K4 removed) the same kernel AUTO / MFMA pick for these shapes */
} psnode_kernel;

/* flags: teacher forcing of my_solvers.py:52 (input_true_x) and :82 (input_true_x, input_true_i) */
#define PSNODE_FLAG_INPUT_TRUE_X 1u
#define PSNODE_FLAG_INPUT_TRUE_I 2u

/* An nn.Sequential(Linear, ELU, Linear, ..., Linear) exactly as nn.Linear stores it:
 * weight[l] row-major [out_dim[l], in] (in = in_dim for l = 0, else out_dim[l-1]), bias[l] [out_dim[l]].
 * ELU(alpha=1) follows every layer but the last.
 * Replaces the forward of DE_Func.x_dot / AE_Func.i_calculator
 * (neural_00_ODE_01_no_encode.py:61-68, neural_01_DAE_01_no_encode.py:64-83). */
typedef struct {
    int32_t n_layers;
    int32_t in_dim;
    int32_t out_dim[PSNODE_MAX_LAYERS];
    const float* weight[PSNODE_MAX_LAYERS];
    const float* bias[PSNODE_MAX_LAYERS];
} psnode_mlp_f32;

/* strided time-major view [T,B,D], element strides, last dim contiguous */
typedef struct {
    const float* ptr;
    int64_t stride_t;
    int64_t stride_b;
} psnode_view_f32;

/* Arguments of FixedGridODESolver.integrate_ODE (my_solvers.py:52-80) with a recognised DE_Func
 * (neural_00_ODE_01_no_encode.py:58-68; latent variant neural_00_ODE_02_direct_encode.py:49-57).
 *
 *   xs[0] = x[0];  for k in 0..T-2:  dt = t[k+1]-t[k];
 *     zk  = event_idx[k] >= 0 ? z_jump[:, event_idx[k]] : z[k]
 *     src = INPUT_TRUE_X ? x[k] : xs[k];   xs[k+1] = src + step(method, f(. ; zk), dt, src)
 *   f(x; z) = MLP_de( cat(a0, cat(x,z) - a0, cat(x,z)) ),  a0 = all_initial
 */
typedef struct {
    int32_t method;            /* psnode_method */
    int32_t kernel;            /* psnode_kernel */
    uint32_t flags;            /* PSNODE_FLAG_INPUT_TRUE_X */
    int32_t x_dim, z_dim;
    int64_t T, B;
    psnode_mlp_f32 de;         /* in_dim must equal 3*(x_dim+z_dim), last out_dim must equal x_dim */
    psnode_view_f32 t;         /* [T,B,1] */
    psnode_view_f32 x;         /* [T,B,x_dim]; only x[0] is read unless INPUT_TRUE_X */
    psnode_view_f32 z;         /* [T,B,z_dim] */
    const float* all_initial;  /* [B, x_dim+z_dim] contiguous */
    const int32_t* event_idx;  /* int32[T-1], -1 = no event at that step; NULL = no events */
    const float* z_jump;       /* [B,nE,z_dim] : z_jump[b*zj_stride_b + e*zj_stride_e + d] */
    int64_t zj_stride_b, zj_stride_e;
    float* x_out;              /* [T,B,x_dim] contiguous (my_solvers.py:62) */
    /* Training forward (ABI 3, optional, both NULL = off): what autograd would save for loss.backward() -- the hidden activations of the
     * three ELU layers per (step, stage, trajectory) and the stage inputs -- written by the integrator itself so that the backward
     * (psnode_ode_backward_f32 with saved_act / saved_xstage) does not recompute the stage evaluations (a third of its MFMA work):
     *   save_act    [T-1, S, 3, B, Hp]   Hp = hidden rounded up to 32 / 64 / 128 (psnode_ode_save_hidden), S = stages of the method
     *   save_xstage [T-1, S, B, x_dim]
     * 6 KB per state-step at hidden 128: sized for the 288 GB of an MI355X, meant for the widths where the recompute is what bounds the
     * training step.  Only the MFMA integrator K1 writes them (psnode_ode_save_hidden() > 0, no teacher forcing): else UNSUPPORTED. */
    float* save_act;
    float* save_xstage;
} psnode_ode_args_f32;

/* Arguments of FixedGridODESolver.integrate_DAE (my_solvers.py:82-131) with recognised DE_Func/AE_Func
 * (neural_01_DAE_01_no_encode.py:61-83; latent variant neural_01_DAE_02_direct_encode.py:70-100).
 *
 *   x0 = x_init; i0 = g(TRUE_X ? x[0] : x0; z[0], v[0]);  xs[0]=x0; is[0]=i0
 *   for k: [event: zk,vk <- jumps; i0 = g(x0; zk, vk)]
 *          x1 = step(f(. ; zk, vk, TRUE_I ? i[k] : i0), start = TRUE_X ? x[k] : x0)
 *          i1 = g(TRUE_X ? x[k+1] : x1; z[k+1], v[k+1]);  xs[k+1]=x1; is[k+1]=i1; x0=x1; i0=i1
 *   f = MLP_de(cat(a0, s-a0, s)), s = cat(x,z,v,i);   g = MLP_ae(cat(a0, x, z, v))
 */
typedef struct {
    int32_t method, kernel;
    uint32_t flags;            /* PSNODE_FLAG_INPUT_TRUE_X | PSNODE_FLAG_INPUT_TRUE_I */
    int32_t x_dim, z_dim, v_dim, i_dim;
    int64_t T, B;
    psnode_mlp_f32 de;         /* in_dim = 3*(x+z+v+i), out = x_dim */
    psnode_mlp_f32 ae;         /* in_dim = (x+z+v+i) + (x+z+v), out = i_dim */
    psnode_view_f32 t, x, z, v, i;   /* x, i only read under teacher forcing (may be NULL otherwise) */
    const float* x_init;       /* [B,x_dim] contiguous */
    const float* all_initial;  /* [B, x+z+v+i] contiguous */
    const int32_t* event_idx;  /* as above */
    const float* z_jump;       /* [B,nE,z_dim] */
    int64_t zj_stride_b, zj_stride_e;
    const float* v_jump;       /* [B,nE,v_dim] */
    int64_t vj_stride_b, vj_stride_e;
    float* x_out;              /* [T,B,x_dim] contiguous */
    float* i_out;              /* [T,B,i_dim] contiguous */
    /* Optional training side outputs, all of them or none (as psnode_ode_args_f32::save_act): what loss.backward() would have autograd
     * keep, so that the backward call (psnode_dae_bwd_wide_args_f32::saved_*) does not recompute the forward:
     *   save_act    [T-1, S, L, B, Hp]   the DE's ELU outputs per (step, stage); Hp = psnode_dae_save_hidden(), L = hidden layers of the MLPs
     *   save_xstage [T-1, S, B, x_dim]   the DE's stage inputs
     *   save_ae_act [L, T, B, Hp]        the AE head's ELU outputs per grid point (my_solvers.py:95, :121)
     *   save_ev_act [nE, L, B, Hp]       the same for the event-time heads i0 = g(x_k; jumps) (my_solvers.py:108-110); rows of events no
     *   save_ev_i   [nE, B, W]           step takes are not written.  save_ev_i: i0 -- K2 shapes (L = 3): W = 16, the slot layout of
     *                                    psnode_dae_bwd_wide_args_f32; latent shapes at hidden 64 (L = 1, K3c): W = i_dim = 64.
     * The two event buffers are required only with event_idx.  Only the MFMA integrators K2 and K3c write them, without teacher forcing
     * (psnode_dae_save_hidden() > 0): else UNSUPPORTED. */
    float* save_act;
    float* save_xstage;
    float* save_ae_act;
    float* save_ev_act;
    float* save_ev_i;
} psnode_dae_args_f32;

/* ABI / build identification. */
int32_t psnode_abi_version(void);
const char* psnode_build_info(void);               /* e.g. "psnode_hip gfx950 ..." (static storage) */
const char* psnode_status_string(int32_t status);  /* static storage */

/* Scratch bytes needed by an integrate call with these MLPs (ae may be NULL).  Host-only, no HIP calls. */
size_t psnode_workspace_bytes(const psnode_mlp_f32* de, const psnode_mlp_f32* ae);

/* Replaces ODE_Event.event_fn + jump_change_fn's index search (neural_base.py:52-62, 178-196), resolved
 * once per call on the device instead of one host sync per step:
 *   event_idx[k] = e such that event_times[e*stride_e] == clock[k*stride_k] (exact fp32 equality), else -1
 * for k in [0, n_steps).  `clock` is trajectory 0's time column, `event_times` trajectory 0's event list.
 * If several e match, *dup_flag (optional int32, device) is set to 1 and the first match is used
 * (the reference raises on that input). */
int32_t psnode_event_table_f32(int64_t n_steps, const float* clock, int64_t stride_k,
                               const float* event_times, int64_t stride_e, int32_t n_events,
                               int32_t* event_idx, int32_t* dup_flag, void* stream);

/* Replaces FixedGridODESolver.integrate_ODE (my_solvers.py:52-80) + Euler/Midpoint/RK4._step_func
 * (my_fixed_grid.py:12-59) + DE_Func.forward for the whole batch and all T-1 steps. */
int32_t psnode_ode_integrate_f32(const psnode_ode_args_f32* args, void* workspace, size_t workspace_bytes, void* stream);

/* Replaces FixedGridODESolver.integrate_DAE (my_solvers.py:82-131) + step functions + DE_Func/AE_Func forwards. */
int32_t psnode_dae_integrate_f32(const psnode_dae_args_f32* args, void* workspace, size_t workspace_bytes, void* stream);

/* Row-wise 2-layer ELU-MLP  out[r,:] = W2.ELU(W1.in[r,:] + b1) + b2  over `rows` rows (row strides in elements).
 * Replaces the forward of the direct_encode encoders/decoders nn.Sequential(Linear, ELU, Linear) applied to every
 * (b,t) row: x_encoder / z_encoder / x_decoder (neural_00_ODE_02_direct_encode.py:64-69,74-88) and
 * v_encoder / i_encoder / i_decoder (neural_01_DAE_02_direct_encode.py:107-118,126-152).
 * Supported: hidden width 16 (the scripts' default hidden_dim) or 64 (their debug override), in/out width up to the
 * hidden width -- see psnode_mlp_rows_supported. */
int32_t psnode_mlp_rows_supported(const psnode_mlp_f32* mlp);
/* Input row r sits at in + r * in_row_stride (in_inner_rows == 0), or -- two-level -- at
 *   in + (r / in_inner_rows) * in_outer_stride + (r % in_inner_rows) * in_row_stride      (rows, in_inner_rows < 2^32):
 * the DataLoader's [B,T,D] batch read as the time-major rows r = t * B + b the latent tensors are laid out in (in_inner_rows = B,
 * in_row_stride = T * D, in_outer_stride = D) -- the x.permute(1, 0, 2) of neural_00_ODE_02_direct_encode.py:76 without a copy. */
int32_t psnode_mlp_rows_f32(const psnode_mlp_f32* mlp, int64_t rows, const float* in, int64_t in_row_stride, int64_t in_inner_rows,
                            int64_t in_outer_stride, float* out, int64_t out_row_stride, void* stream);

/* Backward of psnode_mlp_rows_f32: grad_in[r,:] (optional) and the parameter gradients as ONE flat vector in nn.Linear order
 * [W1 (H x in), b1 (H), W2 (out x H), b2 (out)], from the saved input rows and grad_out.  What loss.backward() does for the
 * encoders/decoders of the direct_encode models (neural_00_ODE_02_direct_encode.py:267-275 through :74-88).
 * Deterministic (per-wave partials in `workspace`, summed in a fixed order).  grad_params == NULL: the partials are left unreduced in
 * `workspace` (psnode_mlp_rows_backward_parts(mlp, rows) * param_count floats suffice) for psnode_mlp_rows_reduce_f32 below. */
size_t psnode_mlp_rows_backward_workspace_bytes(const psnode_mlp_f32* mlp, int64_t rows);
int32_t psnode_mlp_rows_backward_f32(const psnode_mlp_f32* mlp, int64_t rows, const float* in, int64_t in_row_stride,
                                     int64_t in_inner_rows, int64_t in_outer_stride, const float* grad_out, int64_t gout_row_stride, float* grad_in, int64_t gin_row_stride,
                                     float* grad_params, void* workspace, size_t workspace_bytes, void* stream);

/* A module applied to SEVERAL row sets in one step (x_encoder over the grid rows and the first row, z_encoder over grid rows, first row and
 * jump rows: neural_00_ODE_02_direct_encode.py:76-82; the decoder over the solution and the reconstruction, :86-88): call
 * psnode_mlp_rows_backward_f32 once per set with grad_params == NULL and `workspace` = that set's slice of ONE partials buffer
 * (psnode_mlp_rows_backward_parts(mlp, rows) vectors of the module's parameter count each, sets side by side), then
 * psnode_mlp_rows_reduce_f32 over all n_parts vectors: the module's gradient, summed in a fixed order (deterministic).  Replaces one
 * two-launch reduction per set and autograd's `add` per parameter tensor and extra use.  (ABI 9) */
int64_t psnode_mlp_rows_backward_parts(const psnode_mlp_f32* mlp, int64_t rows);
size_t psnode_mlp_rows_reduce_workspace_bytes(const psnode_mlp_f32* mlp, int64_t n_parts);   /* (n_parts + 32) * param_count floats */
int32_t psnode_mlp_rows_reduce_f32(const psnode_mlp_f32* mlp, int64_t n_parts, void* workspace, size_t workspace_bytes, float* grad_params,
                                   void* stream);

/* K10 (ABI 10): tall-skinny contraction over rows,  C[m][n] = sum_r A[r][m] * B[r][n]  (+ colsum_a[m] = sum_r A[r][m], optional), on MFMA
 * with the rows as the contraction index: the weight gradients that are not accumulated inside a sweep kernel -- K9w's blocks over its
 * stored rows at the direct_encode models' hidden widths other than 16 / 64 (the scripts' argparse default --hidden 128:
 * neural_00_ODE_02_direct_encode.py:160-162, what loss.backward() forms for de_func there) -- instead of a library GEMM.
 * M, N <= 128 and multiples of 4; lda / ldb (elements) multiples of 4; A, B 16-byte aligned; C row-major [M, N].  Deterministic
 * (per-workgroup partials in `workspace`, summed in a fixed order). */
typedef struct {
    int64_t rows;
    int32_t M, N;
    const float* A;                  /* [rows, M], row stride lda */
    int64_t lda;
    const float* B;                  /* [rows, N], row stride ldb */
    int64_t ldb;
    float* C;                        /* [M, N] */
    float* colsum_a;                 /* [M] or NULL */
} psnode_gemm_tn_args_f32;
int32_t psnode_gemm_tn_supported(const psnode_gemm_tn_args_f32* args);
size_t psnode_gemm_tn_workspace_bytes(const psnode_gemm_tn_args_f32* args);
int32_t psnode_gemm_tn_f32(const psnode_gemm_tn_args_f32* args, void* workspace, size_t workspace_bytes, void* stream);

/* K11 (ABI 10): one linear layer over rows with a fused epilogue,  Y[r][n] = epi(sum_k X[r][k] * Wm[n][k] + bias[n]),  K, N <= 128:
 * the forward AND backward of the direct_encode encoders / decoders (nn.Sequential(Linear, ELU, Linear) over every (b, t) row,
 * neural_00_ODE_02_direct_encode.py:64-69, 74-88) at the hidden widths psnode_mlp_rows_f32 does not carry (the scripts' argparse default
 * --hidden 128), and the row-wise products of the latent-wide backward.  Wm[n][k] = W[n * w_stride_n + k * w_stride_k]: an nn.Linear
 * weight [N, K] as it is (w_stride_n = K, w_stride_k = 1) or read transposed (a [K, N] tensor: w_stride_n = 1, w_stride_k = N).
 * epi: 0 identity, 1 ELU(alpha = 1), 2 multiply by ELU'(Hh[r][n]) where Hh holds ELU OUTPUTS (the delta of a hidden layer).
 * bias may be NULL.  Row strides in elements, ldx >= K, ldy >= N, ldh >= N; no workspace.  Any 4-byte aligned X / Hh / Y is taken:
 * rows are read / written as float4 only where the base pointer is 16-byte aligned and the row stride a multiple of 4. */
typedef struct {
    int64_t rows;
    int32_t K, N;
    const float* X;                  /* [rows, K], row stride ldx */
    int64_t ldx;
    const float* W;
    int64_t w_stride_n, w_stride_k;
    const float* bias;               /* [N] or NULL */
    int32_t epi;
    const float* Hh;                 /* epi == 2: [rows, N], row stride ldh */
    int64_t ldh;
    float* Y;                        /* [rows, N], row stride ldy */
    int64_t ldy;
} psnode_linear_rows_args_f32;
int32_t psnode_linear_rows_supported(const psnode_linear_rows_args_f32* args);
int32_t psnode_linear_rows_f32(const psnode_linear_rows_args_f32* args, void* stream);

/* The RECONSTRUCTION branch of the direct_encode ODE model at hidden 16 as ONE row kernel each way (ABI 9):
 *   x_re = x_decoder(x_encoder(x))        neural_00_ODE_02_direct_encode.py:87     (x_encoder in <= 16 -> 16 -> 16, x_decoder 16 -> 16 -> out <= 16)
 * and its share of loss.backward() (:267-275).  The encoded rows never reach memory: the forward reads x and writes x_re, the backward reads x
 * and dL/dx_re and returns the parameter gradients of BOTH modules as one flat vector
 *   [W1e (16 x in), b1e (16), W2e (16 x 16), b2e (16) | W1d (16 x 16), b1d (16), W2d (out x 16), b2d (out)]        (nn.Linear order)
 * (deterministic: per-wave partials in `workspace`, summed in a fixed order).  Input rows are addressed as in psnode_mlp_rows_f32. */
int32_t psnode_recon_rows_supported(const psnode_mlp_f32* encoder, const psnode_mlp_f32* decoder);
int32_t psnode_recon_rows_f32(const psnode_mlp_f32* encoder, const psnode_mlp_f32* decoder, int64_t rows, const float* in, int64_t in_row_stride,
                              int64_t in_inner_rows, int64_t in_outer_stride, float* out, int64_t out_row_stride, void* stream);
int64_t psnode_recon_rows_param_count(const psnode_mlp_f32* encoder, const psnode_mlp_f32* decoder);
size_t psnode_recon_rows_backward_workspace_bytes(const psnode_mlp_f32* encoder, const psnode_mlp_f32* decoder, int64_t rows);
int32_t psnode_recon_rows_backward_f32(const psnode_mlp_f32* encoder, const psnode_mlp_f32* decoder, int64_t rows, const float* in,
                                       int64_t in_row_stride, int64_t in_inner_rows, int64_t in_outer_stride, const float* grad_out,
                                       int64_t gout_row_stride, float* grad_params, void* workspace, size_t workspace_bytes, void* stream);

/* Backward (discretise-then-optimise) pass through psnode_ode_integrate_f32: what loss.backward() computes when it
 * walks the unrolled T-step autograd graph of integrate_ODE (neural_00_ODE_01_no_encode.py:358-360 through
 * my_solvers.py:66-78), in one launch.  Inputs: the forward arguments, the forward result xs and dL/dxs.
 * Outputs: dL/dx[0], dL/dz (per grid point; steps that took a jump put their gradient into grad_z_jump instead),
 * dL/dall_initial and dL/d(parameters) as ONE flat vector in nn.Linear order
 * [W1 (64 x 3n), b1, W2, b2, W3, b3, W4 (x_dim x 64), b4] (psnode_ode_backward_param_count floats).
 * Kernels: MFMA backwards for the shape classes 3n -> h -> h -> h -> x_dim (h <= 128, x_dim <= 8, z_dim <= 8; K4x / K4f) and the latent
 * 6H -> H -> H with x_dim = z_dim = H in {16, 64} (16-byte aligned rows); the generic backward for any MLP whose activations
 * fit the 160 KB LDS (its parameter-gradient accumulators move to the workspace when they do not).  Teacher forcing: `flags`;
 * t carries no gradient.  Deterministic (per-workgroup partials summed in a fixed order). */
typedef struct {
    int32_t method;
    int32_t kernel;                  /* psnode_kernel: AUTO = MFMA backward when the shape has one (K4x with saved rows at hidden 33..64 up to 4608
                                        trajectories, else K4f), else generic; _MFMA_WAVE / _MFMA_TILE / _MFMA_WIDE force K4x / K4f / K4f */
    int32_t x_dim, z_dim;
    int64_t T, B;
    psnode_mlp_f32 de;
    psnode_view_f32 t, z;
    const float* all_initial;        /* [B, x+z] contiguous */
    const int32_t* event_idx;        /* as in the forward call, or NULL */
    const float* z_jump;
    int64_t zj_stride_b, zj_stride_e;
    int32_t n_events;
    const float* xs;                 /* forward result [T,B,x_dim] contiguous */
    const float* grad_xs;            /* dL/dxs         [T,B,x_dim] contiguous */
    float* grad_x0;                  /* [B,x_dim] */
    float* grad_z;                   /* [T,B,z_dim] contiguous, or NULL */
    float* grad_z_jump;              /* [B,n_events,z_dim] contiguous, zero-initialised by the caller, or NULL */
    float* grad_all_initial;         /* [B, x+z] */
    float* grad_params;              /* flat, psnode_ode_backward_param_count() floats */
    const float* saved_act;          /* ABI 3, optional: what the forward call wrote to save_act / save_xstage (same method, T, B, MLP).  With them the */
    const float* saved_xstage;       /* one-launch backward K4f skips the recompute of the stage evaluations; both NULL = recompute */
    uint32_t flags;                  /* ABI 5: PSNODE_FLAG_INPUT_TRUE_X = backward of a teacher-forced call (my_solvers.py:72-74: every step starts
                                        from the dataset row x[k]): `xs` then holds the DATASET x [T,B,x_dim] contiguous (the forward result is not
                                        needed), no adjoint is carried from step to step, grad_x0 = dL/dxs[0] + the start adjoint of step 0.
                                        Recompute form only (saved_* must be NULL): K4f where kernel != GENERIC and the shape is its (hidden
                                        <= 128, x_dim <= 8), else the generic backward K5 (kernel AUTO / GENERIC; _MFMA_WAVE is refused) */
} psnode_ode_bwd_args_f32;

int32_t psnode_ode_backward_supported(const psnode_ode_bwd_args_f32* args);
int64_t psnode_ode_backward_param_count(const psnode_ode_bwd_args_f32* args);
size_t psnode_ode_backward_workspace_bytes(const psnode_ode_bwd_args_f32* args);
int32_t psnode_ode_backward_f32(const psnode_ode_bwd_args_f32* args, void* workspace, size_t workspace_bytes, void* stream);

/* Backward pass through psnode_dae_integrate_f32 (no teacher forcing; psnode_dae_backward_tf_f32 below has it): loss.backward() through integrate_DAE
 * (neural_01_DAE_01_no_encode.py:422-424 over my_solvers.py:94-129), including the AE head, the feedback of the
 * algebraic variable into the DE input and the event-time recomputation i0 = g(x0; jumps).
 * grad_params_de / grad_params_ae: flat nn.Linear-order vectors (psnode_dae_backward_param_counts). */
typedef struct {
    int32_t method;
    int32_t kernel;                  /* PSNODE_KERNEL_AUTO: an MFMA backward when the shape has one (3n-64-64-64 DE + AE with
                                        x <= 8, z+v+i <= 8; the latent blocks-of-H shapes, H in {16, 64}), else the generic one */
    int32_t x_dim, z_dim, v_dim, i_dim;
    int64_t T, B;
    psnode_mlp_f32 de, ae;
    psnode_view_f32 t, z, v;
    const float* all_initial;        /* [B, x+z+v+i] */
    const int32_t* event_idx;
    const float* z_jump; int64_t zj_stride_b, zj_stride_e;
    const float* v_jump; int64_t vj_stride_b, vj_stride_e;
    int32_t n_events;
    const float* xs;                 /* forward results [T,B,x_dim], [T,B,i_dim] contiguous */
    const float* is;
    const float* grad_xs;            /* dL/dxs, dL/dis (grad_is may be NULL = zeros) */
    const float* grad_is;
    float* grad_x_init;              /* [B,x_dim] */
    float* grad_z;                   /* [T,B,z_dim] or NULL */
    float* grad_v;                   /* [T,B,v_dim] or NULL */
    float* grad_z_jump;              /* [B,n_events,z_dim], zero-initialised by the caller, or NULL */
    float* grad_v_jump;              /* [B,n_events,v_dim], zero-initialised by the caller, or NULL */
    float* grad_all_initial;         /* [B, x+z+v+i] */
    float* grad_params_de;
    float* grad_params_ae;
    /* ABI 4, optional, all or none (the two event buffers only with event_idx): what the forward call wrote to
     * psnode_dae_args_f32::save_* (same method, T, B, MLPs).  Read by K9 (the latent shapes at hidden 64), which then evaluates nothing
     * forwards; UNSUPPORTED for the shapes whose kernel behind this entry point recomputes (K7, K8, K5). */
    const float* saved_act;
    const float* saved_xstage;
    const float* saved_ae_act;
    const float* saved_ev_act;
    const float* saved_ev_i;
} psnode_dae_bwd_args_f32;

int32_t psnode_dae_backward_supported(const psnode_dae_bwd_args_f32* args);
size_t psnode_dae_backward_workspace_bytes(const psnode_dae_bwd_args_f32* args);
int32_t psnode_dae_backward_f32(const psnode_dae_bwd_args_f32* args, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of a teacher-forced integrate_DAE (my_solvers.py:111-121) on the generic backward K5 -- every shape K5 takes untied, it takes
 * teacher-forced (additive in ABI 10: psnode_dae_bwd_args_f32 is unchanged).  flags / x_true / i_true mean what they mean in
 * psnode_dae_bwd_wide_args_f32 below (K7f):
 *   PSNODE_FLAG_INPUT_TRUE_X: the DE of step k starts from x_true[k]; the head at grid point j (i_0 included) reads x_true[j] and its
 *     x-adjoint is dropped; the recomputed head of an event step still reads the running state base.xs[k] -- the only route by which an
 *     adjoint still travels from step to step through x.
 *   PSNODE_FLAG_INPUT_TRUE_I: the DE reads i_true[k], also on event steps; its algebraic adjoint is dropped (the adjoint of is[k] is
 *     grad_is[k] alone) and the event-time head, which then feeds nothing, is neither recomputed nor differentiated.
 * x_true [T,B,x_dim] / i_true [T,B,i_dim]: contiguous dataset rows, required for the flag set; no gradient is formed for them.
 * flags == 0 forwards to psnode_dae_backward_f32.  With flags: base.kernel AUTO or GENERIC, base.saved_* NULL, T >= 2. */
typedef struct {
    psnode_dae_bwd_args_f32 base;
    uint32_t flags;                  /* PSNODE_FLAG_INPUT_TRUE_X | PSNODE_FLAG_INPUT_TRUE_I */
    const float* x_true;
    const float* i_true;
} psnode_dae_bwd_tf_args_f32;

int32_t psnode_dae_backward_tf_supported(const psnode_dae_bwd_tf_args_f32* args);   /* dims only */
size_t psnode_dae_backward_tf_workspace_bytes(const psnode_dae_bwd_tf_args_f32* args);
int32_t psnode_dae_backward_tf_f32(const psnode_dae_bwd_tf_args_f32* args, void* workspace, size_t workspace_bytes, void* stream);

/* The DAE backward at hidden <= 128 (K7f, csrc/psnode_dae_backward_fused.hip): loss.backward() through integrate_DAE
 * (my_solvers.py:94-129) in ONE launch over the whole grid -- per grid point the AE head's adjoint (its output adjoint = dL/dis of that
 * grid point + what the DE of the step starting there returned through its algebraic inputs), per step the DE stages, at event steps the
 * recompute i0 = g(x0; jumps) and its adjoint.  The DE's parameter gradients are accumulated in the kernel (grad_params_de: flat,
 * nn.Linear order W1,b1,..,W4,b4) and the DE's share of the input gradients is written in its final layout:
 *     grad_zv             [T, B, z+v]          dL/d(z | v) through the DE (zero at event steps and at grid point T-1); every entry written
 *     grad_jump           [B, n_events, z+v]   the same for the jump values of the events taken; zero-initialised by the caller
 *     grad_all_initial_de [B, x+z+v+i]         the DE's share of dL/dall_initial
 * carry_x [B,x_dim] (output) = dL/dx_init without dL/dxs[0].
 * "Slot" layout of an algebraic-variable row [.., 16]: slot q < 2(z+v+i) is the DE's external input q of the `s - a0` block (q < z+v+i) or of
 * the `s` block; the adjoint / value of i-dim d sits in slots z+v+d and (z+v+i)+z+v+d (values: equal; adjoints: to be summed by the caller).
 * Unless psnode_dae_backward_wide_ae_floats(args) > 0 (below) the AE head's rows are written for the caller to contract (K7h,
 * psnode_dae_head_grads_f32: AE parameter gradients, the AE's share of the input gradients), row r = grid point r:
 *     ae_act[l], ae_delta[l]    : [T, B, H]  AE head at grid point r (ELU outputs / pre-activation adjoints of hidden layer l = 1..3)
 *     ae_gi                     : [T, B, 16] adjoint of the head's output, slot layout
 *     ev_act[l], ev_delta[l]    : [n_events, B, H] the event-time recompute of event e (written for the events taken)
 *     ev_gi, ev_i               : [n_events, B, 16] its output adjoint and its value i0, slot layout
 * Shape class: de = 3n -> h -> h -> h -> x_dim, ae = n+x+z+v -> h -> h -> h -> i_dim (the same h <= 128), x_dim <= 8, z+v+i <= 8;
 * H = h rounded up to the kernels' 32 / 64 / 128 (columns h..H-1 of the rows are exact zeros: zero-padded units).
 * (ABI <= 7 also had a split form behind this entry point -- adjoint sweep in time chunks + library GEMMs on the host side -- and its
 * ODE counterpart psnode_ode_backward_wide_f32; removed in ABI 8, K4f / K7f cover their shapes.) */
typedef struct {
    int32_t method;
    int32_t x_dim, z_dim, v_dim, i_dim;
    int64_t T, B;
    psnode_mlp_f32 de, ae;
    psnode_view_f32 t, z, v;
    const float* all_initial;        /* [B, x+z+v+i] */
    const int32_t* event_idx;        /* int32[T-1] or NULL */
    const float* z_jump; int64_t zj_stride_b, zj_stride_e;
    const float* v_jump; int64_t vj_stride_b, vj_stride_e;
    int32_t n_events;
    const float* xs;                 /* forward results [T,B,x_dim], [T,B,i_dim] contiguous */
    const float* is;
    const float* grad_xs;            /* dL/dxs [T,B,x_dim] */
    const float* grad_is;            /* dL/dis [T,B,i_dim] or NULL (= zeros) */
    float* carry_x;                  /* [B,x_dim] out */
    float* ae_act[3];
    float* ae_delta[3];
    float* ae_gi;
    float* ev_act[3];
    float* ev_delta[3];
    float* ev_gi;
    float* ev_i;
    float* grad_params_de;           /* required */
    float* grad_zv;
    float* grad_jump;
    float* grad_all_initial_de;
    /* Optional, all of them or none: what the forward call wrote to psnode_dae_args_f32::save_* (same method, T, B,
     * MLPs; the two event buffers with event_idx).  The kernel then evaluates nothing forwards; ae_act / ev_act / ev_i are NOT written
     * (contract over saved_ae_act / saved_ev_act instead). */
    const float* saved_act;
    const float* saved_xstage;
    const float* saved_ae_act;
    const float* saved_ev_act;
    const float* saved_ev_i;
    /* ABI 5, recompute form only (saved_* NULL): backward of a teacher-forced integrate_DAE (my_solvers.py:111-121).
     * PSNODE_FLAG_INPUT_TRUE_X: the DE of step k starts from x_true[k] and the head at grid point j reads x_true[j] (dataset rows
     * [T,B,x_dim] contiguous) -- no adjoint flows from step to step through x except through an event's recomputed i0, whose head reads
     * the RUNNING state xs[k]; PSNODE_FLAG_INPUT_TRUE_I: the DE reads i_true[k] ([T,B,i_dim] contiguous) instead of the head's value --
     * the DE's algebraic adjoint is dropped (the AE -> DE link is cut).  Gradients w.r.t. the dataset rows themselves are not formed. */
    uint32_t flags;
    const float* x_true;
    const float* i_true;
    /* ABI 5, at hidden <= 64 WITH saved activations (psnode_dae_backward_wide_ae_floats(args) > 0; then REQUIRED): the AE head's gradients are
     * formed in the kernel as well -- nothing is left to contract, no head row is written (ae_act / ae_delta / ae_gi / ev_delta / ev_gi may
     * be NULL; ev_act / ev_i are still scratch of the recompute form).  Flat output, h = the MLPs' hidden width, K1a = n + x + z + v:
     *     [ dAW1 (h x K1a) | db1 (h) | dAW2 (h x h) | db2 | dAW3 (h x h) | db3 | P3 (16 x h) | sg (16) ]
     * P3 / sg are per ext SLOT (slot q < ne: the `s - a0` block, ne <= q < 2 ne: the `s` block; an algebraic variable d owns slots
     * nzv + d and ne + nzv + d): dAW4[d] = P3[nzv + d] + P3[ne + nzv + d], db4[d] likewise from sg.  grad_all_initial_de then holds the WHOLE
     * dL/dall_initial and grad_zv / grad_jump the whole dL/d(z|v) (DE + head). */
    float* grad_params_ae_raw;
} psnode_dae_bwd_wide_args_f32;

int32_t psnode_dae_backward_wide_supported(const psnode_dae_bwd_wide_args_f32* args);   /* dims only */
size_t psnode_dae_backward_wide_ae_floats(const psnode_dae_bwd_wide_args_f32* args);     /* floats of grad_params_ae_raw; 0 = head rows + K7h */
size_t psnode_dae_backward_wide_workspace_bytes(const psnode_dae_bwd_wide_args_f32* args);
int32_t psnode_dae_backward_wide_f32(const psnode_dae_bwd_wide_args_f32* args, void* workspace, size_t workspace_bytes, void* stream);

/* K7h: every contraction over the AE head's rows that the fused-DE form of psnode_dae_backward_wide_f32 leaves to the caller, in one
 * launch (no library GEMM): for rows r < R (grid points, or events) and trajectories b, with h_l = act[l] row r (the head's ELU outputs:
 * saved by the forward call or written by the backward call) and delta_l its layer adjoints,
 *     out = [ dAW2 (h x h) | dAW3 (h x h) | P3 (16 x h): gi[slot] (x) h3 | P0 (h x 16): delta1 (x) u | db1 db2 db3 (3 x h) | sum gi (16) ]
 *     sa1[b] = sum_r delta1[r, b]                      (for dL/dall_initial and dAW1's all_initial columns)
 *     grad_zv[r, b, c] = sum_unit AW1[unit][zv_col0 + c] delta1[r, b][unit],  c < n_zv   (row stride 8)
 * with h = hidden (the MLP's real width; rows are Hp = 32 / 64 / 128 floats wide, zero padded), gi / u rows of 16 floats (gi: slot layout
 * of psnode_dae_bwd_wide_args_f32; u: the head's first-layer input columns behind all_initial, x | z | v, zero padded).  Deterministic
 * (per-workgroup partials summed in a fixed order). */
typedef struct {
    int64_t R, B;
    int32_t hidden;
    int32_t n_zv;
    const float* act[3];             /* row r of layer l: act[l] + r * act_row_stride, [B, Hp] */
    int64_t act_row_stride;
    const float* delta[3];           /* [R, B, Hp] */
    const float* gi;                 /* [R, B, 16] */
    const float* u;                  /* [R, B, 16] */
    const float* aw1;                /* the AE's first nn.Linear weight [hidden, aw1_cols] (read for grad_zv only) */
    int32_t aw1_cols, zv_col0;
    float* grad_zv;                  /* [R, B, 8] or NULL */
    float* sa1;                      /* [B, Hp] */
    float* out;                      /* [psnode_dae_head_grads_out_floats(hidden)] */
} psnode_dae_head_grads_args_f32;

int32_t psnode_dae_head_grads_out_floats(int32_t hidden);
size_t psnode_dae_head_grads_workspace_bytes(const psnode_dae_head_grads_args_f32* args);
int32_t psnode_dae_head_grads_f32(const psnode_dae_head_grads_args_f32* args, void* workspace, size_t workspace_bytes, void* stream);

/* Masked, column-weighted squared-error loss of one (prediction, target) pair and its gradient, in one pass:
 *
 *   out[d]   = scale * inv_norm * col_weight[d] * sum_{t,b} mask[t,b,(d)] * (pred[t,b,d] - target[t,b,d])^2     d < D
 *   out[D]   = t0_coef * sum_{b,d} (pred[0,b,d] - target[0,b,d])^2
 *   out[D+1] = sum_d out[d] + out[D]                                                  (the scalar the scripts call backward on)
 *   grad_pred[t,b,d] = d out[D+1] / d pred[t,b,d]                                     (contiguous [T,B,D], optional)
 *
 * This is the step right after the path in the training loops:
 *   `torch.sum(torch.sum(Loss_func(x_pred, x, reduction='none') * mask, dim=1), dim=0) / torch.sum(mask)` summed over d
 *   (neural_00_ODE_01_no_encode.py:353-355) -> mask = the batch's mask, inv_norm = 1/sum(mask), scale = 1;
 *   the DAE's weighted form `(sum(se*mask) + 9*sum(se[:,:,1:2]*mask)) / sum(mask)` and `Loss_func(x[:,0,:], x_pred[:,0,:])`
 *   (neural_01_DAE_01_no_encode.py:414-419) -> col_weight = [1,10,1,...], t0_coef = 1/(B*D);
 *   the direct_encode reconstruction term `Loss_func(x_re, x)` (neural_00_ODE_02_direct_encode.py:269) -> no mask,
 *   scale = 1/(T*B*D).
 * pred/target/mask are logical [T,B,*] views (element strides, last dim contiguous): pred is normally the integrator's
 * time-major output, target/mask the scripts' B-major tensors.  mask_width: 0 = no mask, 1 = [T,B,1], D = [T,B,D].
 * inv_norm is a DEVICE scalar (so that sum(mask) -- or its all-reduce over ranks -- never has to visit the host);
 * NULL = 1.  Deterministic: per-workgroup partial sums are combined in a fixed order (in double). */
typedef struct {
    int64_t T, B;
    int32_t D;
    int32_t mask_width;
    psnode_view_f32 pred, target, mask;
    const float* col_weight;         /* device [D] or NULL (= ones) */
    const float* inv_norm;           /* device scalar or NULL (= 1) */
    float scale;
    float t0_coef;
    float* out;                      /* device [D+2] */
    float* grad_pred;                /* device [T,B,D] contiguous, or NULL */
} psnode_loss_args_f32;

size_t psnode_masked_mse_workspace_bytes(const psnode_loss_args_f32* args);
int32_t psnode_masked_mse_f32(const psnode_loss_args_f32* args, void* workspace, size_t workspace_bytes, void* stream);

/* K6 with another pointwise loss (additive, same ABI version): with e = pred - target,
 *   PSNODE_LOSS_MSE        rho = e^2                                                   rho' = 2e
 *   PSNODE_LOSS_L1         rho = |e|                                                   rho' = sign(e), 0 at e == 0 (torch's rule)
 *   PSNODE_LOSS_SMOOTH_L1  rho = |e| < beta ? e^2 / (2 beta) : |e| - beta / 2          rho' = clamp(e / beta, -1, 1)       param = beta > 0
 *   PSNODE_LOSS_HUBER      rho = |e| < delta ? e^2 / 2 : delta * (|e| - delta / 2)     rho' = clamp(e, -delta, delta)      param = delta > 0
 * i.e. torch.nn.functional.mse_loss / l1_loss / smooth_l1_loss / huber_loss, the values `Loss_func`
 * (neural_00_ODE_01_no_encode.py:49) takes.
 *
 * Training form: the contract above with rho in place of the square and rho' in grad_pred -- same args, same out[D+2], same
 * grad_pred, same partial rows: psnode_masked_mse_workspace_bytes(args) is the workspace size of this call as well.  Kind MSE, or a
 * NULL fn, forwards to the squared-error entry point above (bitwise its result).
 *
 * Per-sample evaluation form (all four kinds), the scripts' evalute_model line
 *   `torch.sum(Loss_func(x_pred * mask, x * mask, reduction='none'), dim=1)` (neural_00_ODE_01_no_encode.py:123):
 *   out[b,d] = sum_t rho(pred[t,b,d] * m[t,b,(d)] - target[t,b,d] * m[t,b,(d)])        args->out = device [B,D], contiguous
 * The mask multiplies both operands as written (two rounded products, one rounded subtraction).  Every out[b,d] has one writer and one
 * summation order: bitwise repeatable, no workspace.  col_weight / inv_norm / grad_pred must be NULL, scale 1 and t0_coef 0.
 *
 * Order of the checks, all before any launch: NULL args -> PSNODE_ERR_NULL; a kind outside 0..3, or a parameter of kinds 2 / 3 that is
 * <= 0 or not finite -> PSNODE_ERR_UNSUPPORTED; (per-sample: a weight, norm, scale, t0_coef or grad_pred -> PSNODE_ERR_UNSUPPORTED;)
 * then the checks of the squared-error entry point in its order with its statuses.  The `supported` query answers 1 where the training
 * call gets as far as its workspace check (host only). */
typedef enum { PSNODE_LOSS_MSE = 0, PSNODE_LOSS_L1 = 1, PSNODE_LOSS_SMOOTH_L1 = 2, PSNODE_LOSS_HUBER = 3 } psnode_loss_kind;
typedef struct {
    int32_t kind;                    /* psnode_loss_kind */
    float param;                     /* beta / delta; ignored for MSE, L1 */
} psnode_loss_fn_f32;

int32_t psnode_masked_loss_supported(const psnode_loss_args_f32* args, const psnode_loss_fn_f32* fn);
int32_t psnode_masked_loss_f32(const psnode_loss_args_f32* args, const psnode_loss_fn_f32* fn, void* workspace, size_t workspace_bytes, void* stream);
int32_t psnode_loss_per_sample_f32(const psnode_loss_args_f32* args, const psnode_loss_fn_f32* fn, void* stream);

/* The WHOLE forward of the direct_encode ODE model in one launch -- replaces ODE_Model.forward of
 * neural_00_ODE_02_direct_encode.py:74-89 (hidden_dim = 16, the script's default):
 *
 *   Xh = x_encoder(x); Zh = z_encoder(z); a0 = cat(Xh[0], Zh[0]); Zh_jump = z_encoder(z_jump)
 *   Xh_sol = integrate_ODE(de, t, Xh, Zh, a0, events on Zh_jump)                (my_solvers.py:52-80)
 *   x_pred = x_decoder(Xh_sol);  x_re = x_decoder(Xh)
 *
 * t, x, z are the scripts' RAW tensors as time-major views (permute(1,0,2) of [B,T,*]); z_jump is the RAW [B,nE,z_dim] tensor
 * (encoded in the kernel at the steps that take a jump); event_idx as produced by psnode_event_table_f32.
 * Every MLP is Linear(in,16) ELU Linear(16,out): x_encoder x_dim->16->16, z_encoder z_dim->16->16, x_decoder 16->16->x_dim,
 * de 96->16->16 (x_dim, z_dim <= 16).  Xh, Zh and Xh_sol never reach memory (108 B of HBM traffic per state-step instead of ~490);
 * xh_out (optional) receives the latent trajectory [T,B,16] for callers that want it.  No workspace. */
typedef struct {
    int32_t method;                  /* psnode_method */
    int32_t x_dim, z_dim;
    int64_t T, B;
    psnode_mlp_f32 x_encoder, z_encoder, x_decoder, de;
    psnode_view_f32 t, x, z;         /* [T,B,1], [T,B,x_dim], [T,B,z_dim] */
    const int32_t* event_idx;        /* int32[T-1] or NULL */
    const float* z_jump;             /* raw [B,nE,z_dim] */
    int64_t zj_stride_b, zj_stride_e;
    float* x_pred;                   /* [T,B,x_dim] contiguous */
    float* x_re;                     /* x_re[t*xre_stride_t + b*xre_stride_b + d], or NULL to skip the reconstruction */
    int64_t xre_stride_t, xre_stride_b;
    float* xh_out;                   /* [T,B,16] contiguous or NULL */
} psnode_ode_encoded_args_f32;

int32_t psnode_ode_encoded_supported(const psnode_ode_encoded_args_f32* args);   /* 1 / 0, dims only */
int32_t psnode_ode_encoded_integrate_f32(const psnode_ode_encoded_args_f32* args, void* stream);

/* The whole DAE_Model.forward of neural_01_DAE_02_direct_encode.py:125-153 at its shipped hidden_dim 64 in ONE launch (K3g; ABI 6):
 *   Xh0 = x_encoder(x0)                                   x0 = Init_Func(z[0], v[0], i[0]), computed by the caller (once per batch)
 *   Zh = z_encoder(z) (absent when z_dim == 0), Vh = v_encoder(v), Xh = x_encoder(x), Ih = i_encoder(i)
 *   all_initial = cat(Xh0, Zh[0], Vh[0], Ih[0]);  jumps = z_encoder(z_jump) | v_encoder(v_jump)
 *   (Xh_sol, Ih_sol) = integrate_DAE(x_init = Xh0, latent DE 12H|9H -> H -> H, latent AE 7H|5H -> H -> H)      (my_solvers.py:82-131)
 *   x_pred = x_decoder(Xh_sol), x_pred[0] = x0;  i_pred = i_decoder(Ih_sol);  x_re = x_decoder(Xh);  i_re = i_decoder(Ih)
 * t, x, z, v, i are the scripts' RAW tensors as time-major views; z_jump / v_jump the RAW [B,nE,*] tensors; event_idx as produced by
 * psnode_event_table_f32.  Every encoder is Linear(in,64) ELU Linear(64,64) (x_dim <= 16; z_dim, v_dim, i_dim <= 8), every decoder
 * Linear(64,64) ELU Linear(64,out).  None of the six latent [T,B,64] tensors reaches memory.  x_re / i_re: both or neither (NULL: the
 * reconstruction and the x / i encoders' per-row work are skipped; x may then be NULL too).  Workspace: the packed weight images. */
typedef struct {
    int32_t method;                  /* psnode_method */
    int32_t x_dim, z_dim, v_dim, i_dim;
    int64_t T, B;
    psnode_mlp_f32 x_encoder, z_encoder, v_encoder, i_encoder, x_decoder, i_decoder, de, ae;
    psnode_view_f32 t, x, z, v, i;   /* [T,B,1], [T,B,x_dim], [T,B,z_dim], [T,B,v_dim], [T,B,i_dim] */
    const float* x0;                 /* [B, x_dim] contiguous */
    const int32_t* event_idx;        /* int32[T-1] or NULL */
    const float* z_jump;             /* raw [B,nE,z_dim] */
    int64_t zj_stride_b, zj_stride_e;
    const float* v_jump;             /* raw [B,nE,v_dim] */
    int64_t vj_stride_b, vj_stride_e;
    float* x_pred;                   /* [T,B,x_dim] contiguous */
    float* i_pred;                   /* [T,B,i_dim] contiguous */
    float* x_re;                     /* x_re[t*xre_stride_t + b*xre_stride_b + d], or NULL */
    int64_t xre_stride_t, xre_stride_b;
    float* i_re;                     /* i_re[t*ire_stride_t + b*ire_stride_b + d], or NULL */
    int64_t ire_stride_t, ire_stride_b;
} psnode_dae_encoded_args_f32;

int32_t psnode_dae_encoded_supported(const psnode_dae_encoded_args_f32* args);   /* 1 / 0, dims only */
size_t psnode_dae_encoded_workspace_bytes(const psnode_dae_encoded_args_f32* args);
int32_t psnode_dae_encoded_integrate_f32(const psnode_dae_encoded_args_f32* args, void* workspace, size_t workspace_bytes, void* stream);

/* Adjoint sweep through the latent integrators of the direct_encode models at the hidden widths K9 / K8 do not take (every
 * hidden_dim <= 128 with hidden_dim % 4 == 0 other than 16 / 64 -- the scripts' argparse default --hidden 128; K9w, ABI 7): the
 * sequential half of loss.backward() through integrate_ODE / integrate_DAE (my_solvers.py:66-78, 94-129).  Reads what the forward call
 * saved (psnode_*_integrate_f32 with save_act ...: [T-1,S,B,H] hidden activations, the AE head's [T,B,H] and event [nE,B,H] rows) and
 * writes the rows every parameter / input gradient is a plain contraction over (library GEMMs on the caller's side,
 * py_psnode_amd/fused.py: latent_backward_wide):
 *   gk, d1 [T-1,S,B,H]  adjoint of each stage's RHS value / of its hidden pre-activation        d1s [T-1,B,H]  sum of d1 over the stages
 *   gi, da1 [T,B,H]     (DAE) adjoint of i_k / of the AE head's hidden pre-activation           gi_ev, da1_ev [nE,B,H]  of the event heads
 *   grad_x0 [B,H]       dL/dx_0 (x_init of the DAE, x[0] of the ODE)
 * Every array contiguous and 16-byte aligned; the event rows zero-initialised by the caller (events no step takes stay zero). */
typedef struct {
    int32_t method, hidden, z_dim, dae;      /* z_dim = hidden, or 0 for the DAE without z */
    int64_t T, B;
    psnode_mlp_f32 de, ae;                   /* the latent MLPs (ae unused for the ODE) */
    psnode_view_f32 t;
    const int32_t* event_idx;                /* int32[T-1] or NULL */
    const float *grad_xs, *grad_is;          /* [T,B,H]; grad_is NULL = zeros (or the ODE) */
    const float *saved_act, *saved_ae_act, *saved_ev_act;
    float *gk, *d1, *d1s, *gi, *da1, *gi_ev, *da1_ev, *grad_x0;
} psnode_latent_bwd_wide_args_f32;

int32_t psnode_latent_backward_wide_supported(int32_t hidden, int32_t z_dim, int32_t dae);
size_t psnode_latent_backward_wide_workspace_bytes(int32_t hidden);
int32_t psnode_latent_backward_wide_f32(const psnode_latent_bwd_wide_args_f32* args, void* workspace, size_t workspace_bytes, void* stream);

/* Row width Hp of save_act for these dims (32 / 64 / 128) if an AUTO / MFMA call can save its activations, else 0 (dims only). */
int32_t psnode_ode_save_hidden(const psnode_ode_args_f32* args);
int32_t psnode_dae_save_hidden(const psnode_dae_args_f32* args);

/* Which kernel an AUTO call with these dims (and batch size B) would run: PSNODE_KERNEL_GENERIC, PSNODE_KERNEL_MFMA or -- the
 * one-wave-per-4-trajectories integrators K1x / K2x, hidden <= 64 at up to one wave per SIMD -- PSNODE_KERNEL_MFMA_WAVE. */
int32_t psnode_ode_kernel_for(const psnode_ode_args_f32* args);
int32_t psnode_dae_kernel_for(const psnode_dae_args_f32* args);

/* Hidden-layer activations other than ELU(alpha=1) (additive within ABI 10).  The entry points above are the ELU(1) ones; the _act
 * forms below take one activation per MLP next to the unchanged argument structs.  Every hidden layer of that MLP uses it (the last
 * Linear has none, as in DE_Func / AE_Func).  Derivatives are taken from the layer OUTPUT h (DESIGN.md "Activations"):
 *   PSNODE_ACT_ELU         alpha > 0                     x > 0 ? x : alpha (e^x - 1)               h > 0 ? 1 : h + alpha
 *   PSNODE_ACT_TANH        -                             tanh x                                    1 - h^2
 *   PSNODE_ACT_SIGMOID     -                             1 / (1 + e^-x)                            h (1 - h)
 *   PSNODE_ACT_RELU        -                             max(x, 0)                                 h > 0 ? 1 : 0
 *   PSNODE_ACT_LEAKY_RELU  alpha = negative slope >= 0   x > 0 ? x : alpha x                       h > 0 ? 1 : alpha
 *   PSNODE_ACT_SOFTPLUS    beta > 0, threshold           beta x > threshold ? x : log1p(e^(beta x)) / beta
 *                                                                                                  beta h > threshold ? 1 : 1 - e^(-beta h)
 * The pre-activation family (kind bit 5, value 32, set): no parameters (alpha / beta / threshold are ignored), and the derivative is a
 * function of the PRE-activation u, which K5's pre-activation build keeps in LDS next to each hidden layer's output (DESIGN.md
 * "The pre-activation build"):
 *   PSNODE_ACT_SILU        -                             u sigma(u)                                sigma(u) (1 + u (1 - sigma(u)))
 *   PSNODE_ACT_GELU        -    (erf form)               u Phi(u)                                  Phi(u) + u phi(u)
 *   PSNODE_ACT_GELU_TANH   -                             u (1 + t) / 2,                            (1 + t) / 2 + u (1 - t^2) c (1 + 3 k u^2) / 2
 *                                                        t = tanh(c (u + k u^3)), c = sqrt(2 / pi), k = 0.044715
 *   PSNODE_ACT_MISH        -                             u tanh(sp), sp = log1p(e^u)               tanh(sp) + u (1 - tanh^2(sp)) sigma(u)
 *   (sigma: the logistic function; Phi, phi: the standard normal CDF and density.)
 *   The DE and AE of a DAE may use activations of different families.  Kinds 6..31 and >= 36 are unknown.
 *   The backward of this family needs LDS for u as well (per hidden unit 20 floats on K5's staged path, 16 on its register / streamed
 *   paths, next to the layer outputs), so its _act_supported queries answer from the pre build's own fit, which ends before the other
 *   kinds' does: e.g. hidden 160 x 3 with z_dim 2 fits up to x_dim 24 and not at x_dim 32 (where Tanh still fits).  Such shapes answer 0
 *   and give PSNODE_ERR_UNSUPPORTED.  The forward (K0) needs no u: it fits wherever the other kinds do (DESIGN.md "The pre-activation
 *   build").
 * Rules of every _act entry point:
 *   - a NULL act, or ELU with alpha == 1, is ELU(1): the call behaves exactly like the entry point without _act;
 *   - any other act runs the generic kernels only (K0 forward, K5 backward): `kernel` must be PSNODE_KERNEL_AUTO or _GENERIC (the MFMA
 *     kinds give PSNODE_ERR_UNSUPPORTED), and so are the training side outputs save_* / saved_* and the teacher-forced backward;
 *   - an unknown kind gives PSNODE_ERR_METHOD, a parameter outside its range (or not finite) PSNODE_ERR_DIMS.
 * The _act_supported queries answer 1 / 0 for the same rules (dims only, like the queries without _act); an invalid act is 0.
 * Workspace sizes are those of the entry points without _act. */
typedef enum {
    PSNODE_ACT_ELU = 0, PSNODE_ACT_TANH = 1, PSNODE_ACT_SIGMOID = 2, PSNODE_ACT_RELU = 3, PSNODE_ACT_LEAKY_RELU = 4, PSNODE_ACT_SOFTPLUS = 5,
    PSNODE_ACT_PRE_FAMILY = 32,   /* bit 5: the derivative needs the pre-activation */
    PSNODE_ACT_SILU = 32, PSNODE_ACT_GELU = 33, PSNODE_ACT_GELU_TANH = 34, PSNODE_ACT_MISH = 35
} psnode_act_kind;

typedef struct {
    int32_t kind;          /* psnode_act_kind */
    float alpha;           /* ELU: alpha; LEAKY_RELU: negative slope; otherwise ignored */
    float beta, threshold; /* SOFTPLUS; otherwise ignored */
} psnode_act_f32;

int32_t psnode_ode_integrate_act_supported(const psnode_ode_args_f32* args, const psnode_act_f32* de_act);
int32_t psnode_ode_integrate_act_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, void* workspace, size_t workspace_bytes,
                                     void* stream);
int32_t psnode_dae_integrate_act_supported(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act);
int32_t psnode_dae_integrate_act_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                     void* workspace, size_t workspace_bytes, void* stream);
int32_t psnode_ode_backward_act_supported(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act);
int32_t psnode_ode_backward_act_f32(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, void* workspace, size_t workspace_bytes,
                                    void* stream);
int32_t psnode_dae_backward_act_supported(const psnode_dae_bwd_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act);
int32_t psnode_dae_backward_act_f32(const psnode_dae_bwd_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- Explicit Runge-Kutta tableaus on the generic kernels (additive to ABI 10; DESIGN.md "Runge-Kutta tableaus").
 * Any explicit method of 1..4 stages: a[s][j] (j < s) is the coefficient of slope k_j in the argument of stage s, b[s] the weight of k_s
 * in the update.  One step, in fp32, sums in increasing index, a coefficient that is exactly 0 skipped (its slope is not read):
 *     argument of stage s = x0 + h * sum_{j<s} a[s][j] k_j          new state = x0 + h * sum_s b[s] k_s
 * Everything else of the integrators -- zero-order hold of z | v | i, events, the AE head's slots, both teacher-forcing flags -- is that
 * of the entry points without _rk.  The 3/8 rule, for instance, is stages 4, a21 = 1/3, a31 = -1/3, a32 = 1, a41 = 1, a42 = -1, a43 = 1,
 * b = 1/8, 3/8, 3/8, 1/8; it then agrees with PSNODE_RK4_38 up to the rounding of the two ways to write the sums.
 * Rules of every _rk entry point:
 *   - the `method` field of the args is NOT read; the existing entry points keep rejecting every method outside 0..2;
 *   - they run K0 (forward) and K5 (backward) only, in a build of their own that carries every activation kind (ELU(1), a NULL act, runs
 *     as ELU with alpha = 1): `kernel` must be PSNODE_KERNEL_AUTO or _GENERIC and the save_* / saved_* pointers NULL, else
 *     PSNODE_ERR_UNSUPPORTED; so is a backward call with teacher-forcing flags and an activation other than ELU(1);
 *   - K5's tableau build keeps the pre-activations in LDS like its pre-activation build, for every kind: the backward fits the shapes that
 *     build fits (psnode_*_backward_rk_supported answers for it), a class somewhat smaller than that of the ELU(1) backward;
 *   - a NULL tableau gives PSNODE_ERR_NULL; stages outside 1..4, a coefficient that is not finite, or a non-zero a[s][j] with j >= s
 *     (entries of rows / columns >= stages included) PSNODE_ERR_METHOD; an invalid act its status of the _act entry points.
 * The _supported queries answer 1 / 0 for the same rules (dims only).  Workspaces: psnode_workspace_bytes (forward),
 * psnode_ode_backward_workspace_bytes with any valid method (ODE backward), psnode_dae_backward_rk_workspace_bytes (DAE backward).
 * The DAE backward takes psnode_dae_bwd_tf_args_f32, whose flags may be 0: one entry point for plain and teacher-forced calls. */
typedef struct {
    int32_t stages;        /* 1..4 */
    float a[4][4];         /* strictly lower triangular */
    float b[4];
} psnode_rk_tableau_f32;

int32_t psnode_ode_integrate_rk_supported(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab);
int32_t psnode_ode_integrate_rk_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                    void* workspace, size_t workspace_bytes, void* stream);
int32_t psnode_dae_integrate_rk_supported(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                          const psnode_rk_tableau_f32* tab);
int32_t psnode_dae_integrate_rk_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                    const psnode_rk_tableau_f32* tab, void* workspace, size_t workspace_bytes, void* stream);
int32_t psnode_ode_backward_rk_supported(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab);
int32_t psnode_ode_backward_rk_f32(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                   void* workspace, size_t workspace_bytes, void* stream);
int32_t psnode_dae_backward_rk_supported(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                         const psnode_rk_tableau_f32* tab);
size_t psnode_dae_backward_rk_workspace_bytes(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act,
                                              const psnode_act_f32* ae_act, const psnode_rk_tableau_f32* tab);
int32_t psnode_dae_backward_rk_f32(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                   const psnode_rk_tableau_f32* tab, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Sub-steps per grid interval on the generic kernels (additive to ABI 10; DESIGN.md "Sub-steps per grid interval").
 * With substeps = n every grid interval [t[k], t[k+1]] is integrated in n equal sub-steps of h = (t[k+1] - t[k]) / n (one correctly rounded
 * fp32 division per interval and trajectory).  The interval's external inputs -- z | v of grid point k, or the jumped values on an interval
 * that starts with an event -- are held over all n sub-steps; under PSNODE_FLAG_INPUT_TRUE_X only sub-step 0 starts from the dataset row;
 * under PSNODE_FLAG_INPUT_TRUE_I every sub-step reads i[k].  A DAE that integrates its own algebraic variable re-evaluates the head at the
 * start of every sub-step j >= 1, i = g(state; z | v of the interval): the algebraic variable follows the state inside the interval.
 * Outputs stay on the caller's grid: x_out [T,B,x_dim], i_out [T,B,i_dim].
 * x_sub [T-1, n-1, B, x_dim], contiguous and caller-owned like save_xstage: row (k, j-1) is the start state of sub-step j of interval k,
 * 1 <= j < n.  A forward call writes it when the pointer is not NULL (a training forward); a backward call reads it and never writes it.
 * Rules of every _sub entry point (they take what the _rk entry points take, plus this struct):
 *   - a NULL struct gives PSNODE_ERR_NULL, substeps outside 1..1024 PSNODE_ERR_DIMS;
 *   - substeps == 1 forwards to the _rk entry point (tableau given) or the _act entry point (tableau NULL), x_sub is not touched;
 *   - otherwise: a NULL act is ELU(1); a NULL tableau is the built-in `method` of the args written as its tableau (the 3/8 rule then
 *     differs from PSNODE_RK4_38 by rounding only); the call runs K0 / K5 in a build of their own, so `kernel` must be PSNODE_KERNEL_AUTO
 *     or _GENERIC and the save_* / saved_* pointers NULL (PSNODE_ERR_UNSUPPORTED), a teacher-forced backward needs ELU(1), and the backward
 *     fits the shapes the tableau build fits;
 *   - a backward call with substeps > 1, T >= 2 and a NULL x_sub gives PSNODE_ERR_NULL.
 * Every check returns its status before anything is launched.  The _supported queries answer 1 / 0 for the same rules (dims only; x_sub is
 * not looked at).  Workspaces: those of the _rk entry points (psnode_dae_backward_sub_workspace_bytes for the DAE backward). */
typedef struct {
    int32_t substeps;      /* 1..1024 */
    float* x_sub;          /* [T-1, substeps-1, B, x_dim] or NULL (forward); required by a backward call with substeps > 1 */
} psnode_substeps_f32;

int32_t psnode_ode_integrate_sub_supported(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                           const psnode_substeps_f32* sub);
int32_t psnode_ode_integrate_sub_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                     const psnode_substeps_f32* sub, void* workspace, size_t workspace_bytes, void* stream);
int32_t psnode_dae_integrate_sub_supported(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                           const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub);
int32_t psnode_dae_integrate_sub_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                     const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, void* workspace, size_t workspace_bytes,
                                     void* stream);
int32_t psnode_ode_backward_sub_supported(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                          const psnode_substeps_f32* sub);
int32_t psnode_ode_backward_sub_f32(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                    const psnode_substeps_f32* sub, void* workspace, size_t workspace_bytes, void* stream);
int32_t psnode_dae_backward_sub_supported(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                          const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub);
size_t psnode_dae_backward_sub_workspace_bytes(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act,
                                               const psnode_act_f32* ae_act, const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub);
int32_t psnode_dae_backward_sub_f32(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                    const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, void* workspace, size_t workspace_bytes,
                                    void* stream);

/* ---- Linear interpolation of externals on the generic kernels (additive to ABI 10; DESIGN.md "Linear interpolation of externals on K0 / K5").
 * The entry point itself means "linear": stage s (abscissa c_s = sum_{j<s} a[s][j], summed in increasing index) of sub-step j of interval k
 * reads, for every column of z | v,
 *     theta = (j + c_s) / n,   w = w_L + theta * (w_R - w_L)          (fp32, as written, not contracted)
 * with w_L row k of the dataset (the jumped values on an interval that starts with an event) and w_R row k + 1 of the dataset, never
 * jumped; rows beyond T - 1 are not read.  theta does not depend on the clock.  h, the event table, the event-time head (theta = 0), the
 * head at grid point k + 1 (rows k + 1), the outputs and both teacher-forcing flags are what the _sub entry points define; the algebraic
 * variable is never interpolated; a DAE that integrates its own i evaluates the head in front of sub-step j >= 1 at the state and the
 * z | v of theta = j / n.  A backward call adds (1 - theta) g to the gradient of w_L (row k of grad_z / grad_v, or the event's jump
 * gradient) and theta g to row k + 1; no atomics, bitwise repeatable.
 * Rules (the entry points take exactly what their _sub siblings take):
 *   - a NULL psnode_substeps_f32 means one sub-step; otherwise substeps outside 1..1024 gives PSNODE_ERR_DIMS; every substeps >= 1 runs here;
 *   - a NULL act is ELU(1); a NULL tableau is the built-in `method` of the args written as its tableau;
 *   - `kernel` must be PSNODE_KERNEL_AUTO or _GENERIC and the save_* / saved_* pointers NULL (PSNODE_ERR_UNSUPPORTED); a teacher-forced
 *     backward needs ELU(1); the _supported queries answer for this build's own LDS fit (K0: z_dim + v_dim more rows; K5: three times that);
 *   - a backward call with substeps > 1, T >= 2 and a NULL x_sub gives PSNODE_ERR_NULL.
 * Every check returns its status before anything is launched.  Workspaces: those of the _rk entry points. */
int32_t psnode_ode_integrate_lin_supported(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                           const psnode_substeps_f32* sub);
int32_t psnode_ode_integrate_lin_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                     const psnode_substeps_f32* sub, void* workspace, size_t workspace_bytes, void* stream);
int32_t psnode_dae_integrate_lin_supported(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                           const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub);
int32_t psnode_dae_integrate_lin_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                     const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, void* workspace, size_t workspace_bytes,
                                     void* stream);
int32_t psnode_ode_backward_lin_supported(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                          const psnode_substeps_f32* sub);
int32_t psnode_ode_backward_lin_f32(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                    const psnode_substeps_f32* sub, void* workspace, size_t workspace_bytes, void* stream);
int32_t psnode_dae_backward_lin_supported(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                          const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub);
size_t psnode_dae_backward_lin_workspace_bytes(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act,
                                               const psnode_act_f32* ae_act, const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub);
int32_t psnode_dae_backward_lin_f32(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                    const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, void* workspace, size_t workspace_bytes,
                                    void* stream);

/* ---- Per-trajectory events on the generic kernels (additive to ABI 10; DESIGN.md "Per-trajectory events on K0 / K5").
 * The entry point itself means that the args' event_idx is an int32 [T-1, B] table, row-major [k][b]: the index of the event trajectory b
 * takes at step k, -1 = none.  A trajectory with an index >= 0 reads z_jump[b, idx] / v_jump[b, idx] in place of row k of z / v for that
 * interval (all its sub-steps) and, in a DAE, replaces the algebraic variable it carries by the head at (x_k; the jumped rows); a
 * trajectory with -1 reads the dataset rows and keeps the variable it carries.  That is, trajectory b is computed as the shared rule
 * (psnode_event_table_f32, event_idx [T-1]) computes it in a batch that consists of b alone.  Sub-steps, the tableau, the activations
 * and both teacher-forcing flags are what the _sub entry points define.  A backward call writes a hit trajectory's external adjoint to
 * grad_z_jump / grad_v_jump [b, idx] and zero to row k of grad_z / grad_v, another trajectory's to row k; no atomics, bitwise repeatable.
 * psnode_event_table_pt_f32 builds the table: one thread per (k, b) compares clock[k * stride_k + b * stride_b] with
 * event_times[b * stride_eb + e * stride_e], e < n_events (strides in elements), exact float equality, lowest matching e; an entry that
 * matches no clock value (NaN, the padding of a shorter list) never fires; *dup_flag (may be NULL) is set to 1 if any trajectory has two
 * entries that match one step, and is otherwise left as it is.
 * Rules (the entry points take exactly what their _sub siblings take):
 *   - a NULL psnode_substeps_f32 means one sub-step; otherwise substeps outside 1..1024 gives PSNODE_ERR_DIMS; every substeps >= 1 runs here;
 *   - a NULL act is ELU(1); a NULL tableau is the built-in `method` of the args written as its tableau;
 *   - `kernel` must be PSNODE_KERNEL_AUTO or _GENERIC and the save_* / saved_* pointers NULL (PSNODE_ERR_UNSUPPORTED); a teacher-forced
 *     backward needs ELU(1); the _supported queries answer for the LDS fit, which is the _sub build's;
 *   - a NULL event_idx gives PSNODE_ERR_NULL (event-less calls take the other families); a backward call with substeps > 1, T >= 2 and
 *     a NULL x_sub gives PSNODE_ERR_NULL.
 * Every check returns its status before anything is launched.  Workspaces: those of the _rk entry points, as for the _lin family (the
 * DAE backward's: psnode_dae_backward_rk_workspace_bytes with the same args and acts and any valid tableau -- the size does not depend
 * on the tableau, on the number of sub-steps or on the event table); this family has no query of its own. */
int32_t psnode_event_table_pt_f32(int64_t n_steps, int64_t B, const float* clock, int64_t stride_k, int64_t stride_b,
                                  const float* event_times, int64_t stride_eb, int64_t stride_e, int32_t n_events, int32_t* event_idx,
                                  int32_t* dup_flag, void* stream);
int32_t psnode_ode_integrate_pev_supported(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                           const psnode_substeps_f32* sub);
int32_t psnode_ode_integrate_pev_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                     const psnode_substeps_f32* sub, void* workspace, size_t workspace_bytes, void* stream);
int32_t psnode_dae_integrate_pev_supported(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                           const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub);
int32_t psnode_dae_integrate_pev_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                     const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, void* workspace, size_t workspace_bytes,
                                     void* stream);
int32_t psnode_ode_backward_pev_supported(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                          const psnode_substeps_f32* sub);
int32_t psnode_ode_backward_pev_f32(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                    const psnode_substeps_f32* sub, void* workspace, size_t workspace_bytes, void* stream);
int32_t psnode_dae_backward_pev_supported(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                          const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub);
int32_t psnode_dae_backward_pev_f32(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                    const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, void* workspace, size_t workspace_bytes,
                                    void* stream);

/* ---- Two-step Adams-Bashforth on the generic kernels (additive to ABI 10; DESIGN.md "Adams-Bashforth 2 on K0 / K5").
 * Step k, per trajectory, with h_k = t[k+1] - t[k] and f_k the DE at the inputs Euler's single stage reads (state x_k; row k of z | v or the
 * jumped rows; in a DAE the carried head or the event-time head):
 *     x_{k+1} = x_k + c0 f_k + c1 f_{k-1};   restart (k = 0, an event of the trajectory at step k, h_{k-1} == 0): c0 = h_k, c1 = 0;
 *     otherwise rho = h_k / h_{k-1}, c0 = h_k (1 + rho / 2), c1 = -h_k (rho / 2).
 * Outputs, the heads at the grid points and at an event, and the gradients' destinations are Euler's.  A backward call feeds the DE's VJP of
 * step k the cotangent c0_k g_{k+1} + c1_{k+1} g_{k+2} (g: the total adjoint of a state); no atomics, bitwise repeatable; the clock gets
 * no gradient.  One DE evaluation per step, no sub-steps, no interpolation, no tableau: the args' `method` is not read.
 * event_idx may be NULL (no events); otherwise per_trajectory != 0 says that it is the int32 [T-1, B] table of psnode_event_table_pt_f32
 * (the rule of the _pev family), 0 that it is the shared int32 [T-1] of psnode_event_table_f32.
 * Rules: a NULL act is ELU(1); `kernel` must be PSNODE_KERNEL_AUTO or _GENERIC, the save_* / saved_* pointers NULL and no teacher-forcing
 * flag set -- every teacher-forced step starts from a dataset row, a multistep history does not exist -- (PSNODE_ERR_UNSUPPORTED); the
 * _supported queries answer for the LDS fit, which is the _pev (= _sub) build's.  Every check returns its status before anything is
 * launched.  Workspaces: those of the _rk entry points with a one-stage tableau, as for the _pev family; no query of its own. */
int32_t psnode_ode_integrate_ab_supported(const psnode_ode_args_f32* args, const psnode_act_f32* de_act);
int32_t psnode_ode_integrate_ab_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, int32_t per_trajectory, void* workspace,
                                    size_t workspace_bytes, void* stream);
int32_t psnode_dae_integrate_ab_supported(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act);
int32_t psnode_dae_integrate_ab_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                    int32_t per_trajectory, void* workspace, size_t workspace_bytes, void* stream);
int32_t psnode_ode_backward_ab_supported(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act);
int32_t psnode_ode_backward_ab_f32(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, int32_t per_trajectory, void* workspace,
                                   size_t workspace_bytes, void* stream);
int32_t psnode_dae_backward_ab_supported(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act);
int32_t psnode_dae_backward_ab_f32(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                   int32_t per_trajectory, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Multiple-shooting segments on the generic kernels (additive to ABI 10; DESIGN.md "Multiple-shooting segments on K0 / K5").
 * Grid point k is a restart point iff k > 0 and k % every == 0.  The step that leaves a restart point starts from the dataset row x[k]
 * instead of the running state (its first sub-step only), and in a DAE its DE reads the head at that row, g(x[k]; row k of z | v, or the
 * jumped rows if event_idx[k] >= 0), in place of the algebraic variable it carries.  The outputs x_out[k] / i_out[k] of a restart point
 * stay the previous segment's prediction; every grid-point head reads the running state.  So output rows m every + 1 ..
 * min((m + 1) every, T - 1) are what the _sub call returns in its rows 1 .. on the slices [m every : (m + 1) every + 1] started from
 * x[m every].  A forward call reads the rows from args->x, which must then hold all T of them (an ODE's row 0 is the start of the call,
 * as always; a DAE starts from x_init); a backward call reads them from x_true.  The dataset rows get no gradient: a backward call drops
 * the start adjoint of a restart step and the x part of the restart head's VJP; that head's z | v part goes to row k of grad_z / grad_v, or
 * to the event's jump row; grad_x0 / grad_x_init is segment 0's.  No atomics, bitwise repeatable.  Sub-steps, the tableau, the
 * activations and the shared event table are what the _sub entry points define.
 * Rules (the entry points take what their _sub siblings take, plus the segments struct in front of the workspace):
 *   - a NULL psnode_segments_f32 gives PSNODE_ERR_NULL, every < 1 PSNODE_ERR_DIMS -- before anything else is looked at;
 *   - a NULL psnode_substeps_f32 means one sub-step; a NULL act is ELU(1); a NULL tableau is the built-in `method` of the args;
 *   - `kernel` must be PSNODE_KERNEL_AUTO or _GENERIC, the save_* / saved_* pointers NULL and no teacher-forcing flag set -- every
 *     teacher-forced step restarts already --, and a DAE forward call's x view must not be empty (PSNODE_ERR_UNSUPPORTED); the _supported
 *     queries answer for the LDS fit, which is the _sub build's;
 *   - a backward call with T - 1 > every and a NULL x_true gives PSNODE_ERR_NULL.
 * Every check returns its status before anything is launched.  Workspaces: those of the _rk entry points, as for the _pev family; this
 * family has no query of its own. */
typedef struct {
    int32_t every;         /* >= 1: grid point k > 0 with k % every == 0 restarts from the dataset row */
    const float* x_true;   /* [T,B,x_dim] contiguous dataset rows; read by the backward calls (a forward call reads args->x), may be NULL there */
} psnode_segments_f32;
int32_t psnode_ode_integrate_ms_supported(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                          const psnode_substeps_f32* sub, const psnode_segments_f32* seg);
int32_t psnode_ode_integrate_ms_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                    const psnode_substeps_f32* sub, const psnode_segments_f32* seg, void* workspace, size_t workspace_bytes,
                                    void* stream);
int32_t psnode_dae_integrate_ms_supported(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                          const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_segments_f32* seg);
int32_t psnode_dae_integrate_ms_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                    const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_segments_f32* seg,
                                    void* workspace, size_t workspace_bytes, void* stream);
int32_t psnode_ode_backward_ms_supported(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                         const psnode_substeps_f32* sub, const psnode_segments_f32* seg);
int32_t psnode_ode_backward_ms_f32(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                   const psnode_substeps_f32* sub, const psnode_segments_f32* seg, void* workspace, size_t workspace_bytes,
                                   void* stream);
int32_t psnode_dae_backward_ms_supported(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                         const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_segments_f32* seg);
int32_t psnode_dae_backward_ms_f32(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                   const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_segments_f32* seg,
                                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- Multiple-shooting segments in parallel (additive to ABI 10; DESIGN.md "Segments in parallel on K0 / K5 (BuildMsp)").
 * The _ms call, computed by a launch grid of tiles x C workgroups instead of tiles: the dataset rows get no gradient, so the segments of a
 * record are independent, forward and backward.  A record of T grid points has n_seg = ceil((T - 1) / every) segments; per_group
 * consecutive ones form a time chunk, C = max(1, ceil(n_seg / per_group)) chunks; chunk c covers the steps c per_group every ..
 * min((c + 1) per_group every, T - 1) - 1, and workgroup (tile, c) integrates its 16 trajectories over that chunk alone, or sweeps it
 * backward.  What is computed is the _ms call's: x_out / i_out / x_sub, grad_x0 / grad_x_init, grad_z / grad_v and the jump gradients
 * bit for bit; grad_params and grad_all_initial are sums over tiles x C partials (chunk 0's grad_all_initial plus the later chunks' in
 * ascending order), so they differ from the _ms call's by the order of the additions.  Nothing crosses a chunk border inside a kernel
 * -- no atomics, no flags, no fences: a small launch behind the backward sweep adds the grad_all_initial partials and, for a DAE, the
 * z | v share of the head at a chunk's last grid point onto that row of grad_z / grad_v.  Bitwise repeatable.
 * Rules: those of the _ms entry points with psnode_segment_groups_f32 in the segments struct's place -- NULL gives PSNODE_ERR_NULL,
 * every < 1 or per_group < 1 PSNODE_ERR_DIMS, before anything else is looked at; per_group >= n_seg is legal and runs one chunk; more
 * than 65535 chunks give PSNODE_ERR_UNSUPPORTED.  The forward workspace is psnode_workspace_bytes'; a backward call's is its own query's
 * (one parameter partial per workgroup of the grid, and what crosses the chunk borders), 0 for a call the _supported query refuses. */
typedef struct {
    int32_t every;         /* >= 1: grid point k > 0 with k % every == 0 restarts from the dataset row */
    const float* x_true;   /* as psnode_segments_f32::x_true */
    int32_t per_group;     /* >= 1: segments per time chunk */
} psnode_segment_groups_f32;
int32_t psnode_ode_integrate_msp_supported(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                           const psnode_substeps_f32* sub, const psnode_segment_groups_f32* grp);
int32_t psnode_ode_integrate_msp_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                     const psnode_substeps_f32* sub, const psnode_segment_groups_f32* grp, void* workspace, size_t workspace_bytes,
                                     void* stream);
int32_t psnode_dae_integrate_msp_supported(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                           const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_segment_groups_f32* grp);
int32_t psnode_dae_integrate_msp_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                     const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_segment_groups_f32* grp,
                                     void* workspace, size_t workspace_bytes, void* stream);
int32_t psnode_ode_backward_msp_supported(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                          const psnode_substeps_f32* sub, const psnode_segment_groups_f32* grp);
size_t psnode_ode_backward_msp_workspace_size(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                              const psnode_substeps_f32* sub, const psnode_segment_groups_f32* grp);
int32_t psnode_ode_backward_msp_f32(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                    const psnode_substeps_f32* sub, const psnode_segment_groups_f32* grp, void* workspace, size_t workspace_bytes,
                                    void* stream);
int32_t psnode_dae_backward_msp_supported(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                          const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_segment_groups_f32* grp);
size_t psnode_dae_backward_msp_workspace_size(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                              const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub,
                                              const psnode_segment_groups_f32* grp);
int32_t psnode_dae_backward_msp_f32(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                    const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_segment_groups_f32* grp,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- Three-step Adams-Bashforth with a predictor-corrector restart step on the generic kernels (additive to ABI 10; DESIGN.md
 * "Adams-Bashforth 3 on K0 / K5").  Step k, per trajectory, with h_k = t[k+1] - t[k] and f_k the DE at the inputs the _ab family's stage reads.
 * Restart flag R_k: k = 0, an event of the trajectory at step k, or h_{k-1} == 0.  Depth d_k: 0 if R_k; 1 if R_{k-1} or
 * h_{k-1} + h_{k-2} == 0; 2 otherwise.
 *     d_k = 2, h0, h1, h2 = h_k, h_{k-1}, h_{k-2}:  g1 = h0^2 / 2, g2 = h0^3 / 3 + h1 g1, D = g2 / (h1 + h2),
 *              c0 = h0 + g1 / h1 + D / h1, c1 = -g1 / h1 - D / h1 - D / h2, c2 = D / h2;   x_{k+1} = x_k + c0 f_k + c1 f_{k-1} + c2 f_{k-2}
 *     d_k = 1: the _ab family's step.
 *     d_k = 0: x~ = x_k + h f_k;  f~ = the DE at (x~; rows k + 1 of z | v, never jumped; a DAE: i~ = AE(x~; z[k+1], v[k+1]), no output);
 *              x_{k+1} = x_k + (h / 2)(f_k + f~);  the slope kept for the history is f_k.
 * Outputs, the heads at the grid points and at an event are the _ab family's.  A backward call runs the corrector's VJP in front of the
 * DE's on a restart step and adds its z | v part to row k + 1 of grad_z / grad_v; the DE's VJP of step k takes
 * a_k g_{k+1} + c1_{k+1} g_{k+2} + c2_{k+2} g_{k+3} (+ h (df~/dx~)^T (h / 2) g_{k+1} on a restart step, where a_k = h / 2).  No atomics,
 * bitwise repeatable; the clock gets no gradient.  Rows beyond T - 1 are never read.
 * Arguments, rules, the order of checks and the workspaces are the _ab family's, prototype for prototype. */
int32_t psnode_ode_integrate_ab3_supported(const psnode_ode_args_f32* args, const psnode_act_f32* de_act);
int32_t psnode_ode_integrate_ab3_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, int32_t per_trajectory, void* workspace,
                                     size_t workspace_bytes, void* stream);
int32_t psnode_dae_integrate_ab3_supported(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act);
int32_t psnode_dae_integrate_ab3_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                     int32_t per_trajectory, void* workspace, size_t workspace_bytes, void* stream);
int32_t psnode_ode_backward_ab3_supported(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act);
int32_t psnode_ode_backward_ab3_f32(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, int32_t per_trajectory, void* workspace,
                                    size_t workspace_bytes, void* stream);
int32_t psnode_dae_backward_ab3_supported(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act);
int32_t psnode_dae_backward_ab3_f32(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                    int32_t per_trajectory, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Four-point Lagrange interpolation of z | v inside every grid interval on the generic kernels (additive to ABI 10; DESIGN.md
 * "Lagrange externals on K0 / K5").  The _lin family with another interpolant: stage s of sub-step j of interval k reads, per trajectory
 * and per column of z | v,
 *     w(theta) = sum_{m < q} l_m(off + theta) node_{s+m},   l_m(u) = prod_{r != m, r < q} (u - r) / (m - r),   theta = (j + c_s) / substeps,
 * the polynomial through q = 2 .. 4 consecutive dataset rows s .. s + q - 1, taken as equally spaced, with s = k - off.  Node s is the
 * jumped row (z_jump / v_jump of event_idx[s]) where event_idx[s] >= 0, every other node the dataset row.  At theta = 0 and 1 the weights
 * are exactly 0 / 1.  q and off come from the stencil table, one code byte per grid interval and trajectory:
 *     psnode_ext_stencil_f32 table[(T - 1) * B], row-major [T-1, B];   code = off | (q << 2),   off = code & 3,   q = (code >> 2) & 7.
 * The table's author (py_psnode_amd.fused.lagrange_stencils) cuts every trajectory's record into pieces -- maximal runs of intervals with
 * t[k+1] > t[k] and no event step inside -- and gives interval k of piece [a, e] q = min(4, e - a + 1), s = clamp(k - 1, a, e - q + 1); an
 * interval with t[k+1] <= t[k] is a piece of its own (q = 2, off = 0).  A NULL table is one piece 0 .. T - 1 for every trajectory:
 * q = min(4, T), s = clamp(k - 1, 0, T - q).  The kernels clamp q to 2 .. min(4, T) and s to 0 .. T - q, so no byte makes them read
 * outside rows 0 .. T - 1.  A backward call adds l_m(u) times a stage's external adjoint to row s + m of grad_z / grad_v (to the jump
 * gradient of event_idx[s] for a jumped node s), by the thread that owns the element: no atomics, bitwise repeatable; it zeroes every
 * row of grad_z / grad_v / grad_z_jump / grad_v_jump itself.  The clock gets no gradient.
 * Everything else -- h, sub-steps, tableau, activations, teacher forcing, the heads, x_sub, the statuses and their order, the workspaces --
 * is the _lin family's, prototype for prototype plus the table; psnode_dae_backward_lag_workspace_size is the family's workspace query
 * (bytes; what psnode_dae_backward_lin_workspace_bytes is to _lin). */
typedef int8_t psnode_ext_stencil_f32;
#define PSNODE_STENCIL_CODE(off, q) ((psnode_ext_stencil_f32)((off) | ((q) << 2)))
#define PSNODE_STENCIL_OFF(code) ((code) & 3)
#define PSNODE_STENCIL_Q(code) (((code) >> 2) & 7)
int32_t psnode_ode_integrate_lag_supported(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                           const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* stencil);
int32_t psnode_ode_integrate_lag_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                     const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* stencil, void* workspace,
                                     size_t workspace_bytes, void* stream);
int32_t psnode_dae_integrate_lag_supported(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                           const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub,
                                           const psnode_ext_stencil_f32* stencil);
int32_t psnode_dae_integrate_lag_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                     const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* stencil,
                                     void* workspace, size_t workspace_bytes, void* stream);
int32_t psnode_ode_backward_lag_supported(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                          const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* stencil);
int32_t psnode_ode_backward_lag_f32(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, const psnode_rk_tableau_f32* tab,
                                    const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* stencil, void* workspace,
                                    size_t workspace_bytes, void* stream);
int32_t psnode_dae_backward_lag_supported(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                          const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub,
                                          const psnode_ext_stencil_f32* stencil);
size_t psnode_dae_backward_lag_workspace_size(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act,
                                              const psnode_act_f32* ae_act, const psnode_rk_tableau_f32* tab,
                                              const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* stencil);
int32_t psnode_dae_backward_lag_f32(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                    const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* stencil,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- Stabilised explicit steps (Runge-Kutta-Chebyshev recurrences) on the generic kernels (additive to ABI 10; DESIGN.md
 * "Runge-Kutta-Chebyshev steps on K0 / K5").  Every grid interval is ONE step of `stages` right-hand-side evaluations, h = t[k+1] - t[k]:
 *     Y_0 = the step's start state, F_0 = F(Y_0);   Y_1 = Y_0 + (mu_t[0] h) F_0;
 *     Y_j = kappa[j-1] Y_0 + mu[j-1] Y_{j-1} + nu[j-1] Y_{j-2} + (mu_t[j-1] h) F(Y_{j-1}) + (gamma_t[j-1] h) F_0,   j = 2 .. stages
 * summed in the order written, a coefficient that is exactly 0 skipped, fp32, not contracted; the new state is Y_stages.  The externals are
 * held (the jumped rows behind an event); a DAE that integrates its own i evaluates the head at (Y_{j-1}; z_k, v_k) in front of every
 * stage j >= 2, as the _sub family does in front of its sub-steps; F_0 is the first stage's evaluation, reused.  x_stage keeps Y_1 ..
 * Y_{stages-1} of every interval (row (k, j - 1): Y_j), written by a forward call where the pointer is not NULL, read by a backward call.
 * The entry points take what their _sub siblings take with this struct in the sub-steps struct's place and no tableau; the order of the
 * checks and the statuses are that family's: a NULL struct is PSNODE_ERR_NULL, stages outside 1..PSNODE_RKC_MAX_STAGES PSNODE_ERR_DIMS
 * (the coefficients are not looked at: index 0 of kappa / mu / nu / gamma_t is never read); a backward call with stages > 1, T >= 2 and a
 * NULL x_stage is PSNODE_ERR_NULL; every check returns before a launch.  No stage count forwards to another family.  The backward runs
 * the recurrence's adjoint stage by stage, last to first; no atomics, bitwise repeatable.  Workspaces: those of the _rk entry points
 * (psnode_dae_backward_rkc_workspace_size for the DAE backward, in bytes). */
#define PSNODE_RKC_MAX_STAGES 32
typedef struct {
    int32_t stages;                          /* 1..PSNODE_RKC_MAX_STAGES */
    float kappa[PSNODE_RKC_MAX_STAGES];      /* entry j - 1: the coefficient of stage j */
    float mu[PSNODE_RKC_MAX_STAGES];
    float nu[PSNODE_RKC_MAX_STAGES];
    float mu_t[PSNODE_RKC_MAX_STAGES];
    float gamma_t[PSNODE_RKC_MAX_STAGES];
    float* x_stage;                          /* [T-1, stages-1, B, x_dim] or NULL (forward); required by a backward call with stages > 1 */
} psnode_rkc_f32;
int32_t psnode_ode_integrate_rkc_supported(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rkc_f32* rkc);
int32_t psnode_ode_integrate_rkc_f32(const psnode_ode_args_f32* args, const psnode_act_f32* de_act, const psnode_rkc_f32* rkc, void* workspace,
                                     size_t workspace_bytes, void* stream);
int32_t psnode_dae_integrate_rkc_supported(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                           const psnode_rkc_f32* rkc);
int32_t psnode_dae_integrate_rkc_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                     const psnode_rkc_f32* rkc, void* workspace, size_t workspace_bytes, void* stream);
int32_t psnode_ode_backward_rkc_supported(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, const psnode_rkc_f32* rkc);
int32_t psnode_ode_backward_rkc_f32(const psnode_ode_bwd_args_f32* args, const psnode_act_f32* de_act, const psnode_rkc_f32* rkc, void* workspace,
                                    size_t workspace_bytes, void* stream);
int32_t psnode_dae_backward_rkc_supported(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                          const psnode_rkc_f32* rkc);
size_t psnode_dae_backward_rkc_workspace_size(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act,
                                              const psnode_act_f32* ae_act, const psnode_rkc_f32* rkc);
int32_t psnode_dae_backward_rkc_f32(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                    const psnode_rkc_f32* rkc, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Stage-wise algebraic heads for Runge-Kutta DAE steps on the generic kernels (additive to ABI 10; DESIGN.md "Stage-wise algebraic
 * heads on K0 / K5").  The _lin / _lag families freeze a DAE's algebraic variable i over the stages of a (sub-)step, as the reference does;
 * this family evaluates it at every stage, the standard treatment of an index-1 DAE.  Interval k, n sub-steps, sub-step j, stage s with
 * abscissa c_s and theta_s = (j + c_s) / n:
 *     stage 0 reads the i it reads in _lin / _lag: the carried head of grid point k, the event-time head on the jumped rows, and for
 *     j >= 1 the in-interval head at theta = j / n;
 *     stage s >= 1, X_s = x + h sum_{j' < s} a[s][j'] k_j', (z_s, v_s) the interpolant at theta_s (the rows its DE stage reads):
 *         i_s = g(X_s, z_s, v_s, all_initial),   k_s = f(X_s, z_s, v_s, i_s)   -- one more AE evaluation per stage, no output row.
 * The head at grid point k + 1, both outputs, h, the event table, theta and the interpolants are untouched.  Under
 * PSNODE_FLAG_INPUT_TRUE_I every stage reads i_true[k] and no head runs inside an interval, and a one-stage tableau has no stage s >= 1:
 * both calls compute what their _lin / _lag siblings compute.  A DAE only: an ODE has no head.
 * The entry points take what their _lag siblings take plus `interp` behind the stencil table, which picks the interpolant:
 * PSNODE_EXT_LINEAR (the straight line of the _lin family; the table is not read) or PSNODE_EXT_LAGRANGE (the polynomial of the _lag family
 * through the table's stencils; NULL: one piece).  Any other value is PSNODE_ERR_METHOD in front of every other check (the queries: 0);
 * behind it the order of the checks and the statuses are the _lin / _lag family's, and every check returns before a launch.  LDS fit and
 * workspaces are those siblings' (no LDS of its own: K5 recomputes a stage's i in front of its VJP); psnode_dae_backward_sth_workspace_size is
 * the family's workspace query (bytes; named as psnode_dae_backward_lag_workspace_size is).  The backward sends the i part of the
 * DE's VJP of a stage s >= 1 through the head's VJP at (X_s, the externals at theta_s): its x part joins the adjoint of X_s, its z | v part
 * goes where the stage's own external adjoint goes, all_initial and the AE's parameters where the in-interval head's go.  Fixed
 * ownership, no atomics, bitwise repeatable.  The clock gets no gradient. */
#define PSNODE_EXT_LINEAR 1
#define PSNODE_EXT_LAGRANGE 2
int32_t psnode_dae_integrate_sth_supported(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                           const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub,
                                           const psnode_ext_stencil_f32* stencil, int32_t interp);
int32_t psnode_dae_integrate_sth_f32(const psnode_dae_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                     const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* stencil,
                                     int32_t interp, void* workspace, size_t workspace_bytes, void* stream);
int32_t psnode_dae_backward_sth_supported(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                          const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub,
                                          const psnode_ext_stencil_f32* stencil, int32_t interp);
size_t psnode_dae_backward_sth_workspace_size(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act,
                                              const psnode_act_f32* ae_act, const psnode_rk_tableau_f32* tab,
                                               const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* stencil, int32_t interp);
int32_t psnode_dae_backward_sth_f32(const psnode_dae_bwd_tf_args_f32* args, const psnode_act_f32* de_act, const psnode_act_f32* ae_act,
                                    const psnode_rk_tableau_f32* tab, const psnode_substeps_f32* sub, const psnode_ext_stencil_f32* stencil,
                                    int32_t interp, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PSNODE_HIP_H */
