/* fabind_hip.h -- C ABI of libfabind_hip.so: the MI355X (gfx950) kernels behind the FABind docking hot path.
 *
 * The reference (QizhiPei/FABind) is 100 % Python; its "native layer" is ATen + torch_scatter +
 * torch_geometric ops called from fabind/models/*.py.  Each entry point below replaces the group of
 * those ops named in its comment (paths relative to the reference's FABind/fabind directory).  Plain pointers
 * and sizes only: every pointer is a DEVICE pointer unless stated otherwise, `stream` is a
 * hipStream_t, dtype codes are FB_DT_F32 = 0 / FB_DT_BF16 = 1 (raw bfloat16 bits), activation
 * codes FB_ACT_NONE/SILU/RELU/SIGMOID = 0..3 (4 = FB_ACT_STORED_DERIV: the aux operand already is the derivative).  Every function returns 0 on success, non-zero on
 * error (message via fabind_last_error()); none of them synchronises or allocates.
 *
 * Node layout contract: nodes are complex-contiguous in the fixed order
 * [glb_c, ligand atoms..., glb_p, protein residues...]; node_off[b] is the first node of complex b
 * (node_off[B] = N) and c_cnt[b] = Nc_b + 1 the size of the ligand-side block (global node included).
 */
#ifndef FABIND_HIP_H
#define FABIND_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_PLATFORM_AMD__
typedef struct ihipStream_t* hipStream_t;
#endif

const char* fabind_last_error(void);
/* Bumped whenever an entry point's signature or an argument struct's layout changes.  History: 1 = first round-1 layout;
 * 2 = FabindGemmArgs grew {p_drop, drop_seed, row_mu, row_rs, col_c}, FabindEdgeBwdArgs / FabindPairUpdateArgs added;
 * 3 = fabind_cross_attn_bwd takes a scratch buffer instead of (n_q_rows, n_k_rows), fabind_cross_attn_bwd_scratch added;
 * 4 = fabind_pair_bias_cat takes a colpart argument (per-work-group column sums), fabind_pair_bias_cat_parts and the
 *     fabind_gemm_tn_set_waves knob added.
 * 5 = FabindGemmArgs grew {C16, ldc16}; fabind_cross_attn_mfma_fwd / fabind_cross_attn_mfma_bwd added (MFMA bf16 form of the cross attention); FabindEdgeBwdArgs grew
 *     bnd + d2scratch, fabind_gcl_edge_fused takes bnd (deterministic boundary sums instead of float atomics), fabind_gcl_edge_fused_bwd_set_variant / _variant added.
 * 6 = bf16 result copies emitted by their producers (no cast kernels): fabind_segment_sum takes (out16, ldo16), fabind_gcl_edge_fused takes agg16, fabind_inter_attn_fwd takes h16,
 *     FabindEdgeBwdArgs grew {dAB16, lddab16}; fabind_gcl_edge_fused_set_variant / _variant (forward kernel form) added.
 * 7 = fabind_multi_copy + FabindCopySeg added (the parameter pack and its adjoint as one launch each).
 * 8 = fabind_split_sum added (split-contraction partials reduced straight into fp32 or bf16).
 * 9 = fabind_zero_empty_rows added (outputs of the fused edge kernels are no longer memset whole).
 * 10 = fabind_gemm_tn_tile_n added (the host sizes the split count of fabind_gemm_tn from the output tile of the current layout: 256 x 256 on
 *     eight waves by default); knobs fabind_gemm_tn_set_exp, fabind_gemm_set_small_m; fabind_gemm_tn_set_waves accepts 16 / 20.
 * 12: fabind_mul_dact / fabind_mul_dact_colsum take `scale` (ReLU + epilogue dropout under autograd);
 *     fabind_cross_attn_fused_fwd / fabind_pair_bo_pack (pair bias recomputed inside the attention kernel), fabind_pair_hadamard_bwd_grid;
 *     FabindGemmArgs.split3 (fp32 x fp32 contracted as split bf16, three MFMAs per product term: precision mode 'bf16x3');
 *     fabind_gcl_edge_fused_x3 (the fused forward edge pipeline in that arithmetic); knob fabind_gemm_set_x3_tile.
 * 11 = fabind_gemm_tn takes with_colsum (the bias gradient rides along with the weight gradient: no separate column-sum launches);
 *     fabind_split_sum takes (n_tail, out_tail); fabind_inter_attn_bwd writes wpart as [nblk][4][H] (was [4][nblk][H]);
 *     fabind_pair_hadamard_bwd_rows added (the pair-Hadamard adjoint over the inter graph without float atomics);
 *     fabind_layernorm_rows_bwd takes nblk (the caller sizes the partial buffers; the kernel strides rows over that grid).
 * 13 = FabindGemmArgs.r_dtype (bf16 residual operand).  14 = fabind_rows_hadamard_bwd, fabind_node_chain_fwd added.
 * 15 = fabind_gemm_tn_multi + FabindTnJob (the queued weight-gradient contractions of a backward pass as one launch + one reduction);
 *     fabind_sizeof_args(3) = sizeof(FabindTnJob); fabind_gcl_edge_fused_x3 takes n_rows (4 GiB bound of its 32-bit gather offsets checked);
 *     fabind_pair_bias_finish writes per-work-group partials of dw (no float atomics; the caller sums them with fabind_colsum);
 *     fabind_pack_frag_multi + FabindPackSeg (all fragment packs of a model call in one launch); fabind_lower_bound;
 *     fabind_cross_attn_fused_fwd takes lse; fabind_cross_attn_fused_bwd + FabindAttnFusedBwdArgs, fabind_pair_bot_pack (fused backward of the
 *     cross attention: fabind_sizeof_args(4)).
 * 16 = fabind_gcl_edge_fused_train (the forward that saves M / silu'(pre2) / pre3) and FabindEdgeBwdArgs.{d2f, z3f} (the two-contraction backward).
 * 17 = round-5 retirement of knob-only kernels: fabind_gemm_set_big removed (256 x 256 GEMM tiles); fabind_gcl_edge_fused_set_variant accepts 1 only,
 *     fabind_gcl_edge_fused_bwd_set_variant 0 / 5 only, fabind_gcl_edge_fused_bwd_set_tile 64 only (their other kernels are no longer built);
 *     fabind_gcl_edge_fused_x3_train added (the split-bf16 forward that saves M / silu'(pre2) / pre3 for the two-contraction backward);
 *     fabind_inter_attn_fwd_rows / fabind_inter_attn_bwd_rows added (inter-edge attention with the rows dealt by degree: heavy rows on four waves);
 *     fabind_edge_lnfold_bwd (+ _blocks) added (FABind+: the LayerNorm-folded first edge Linear under autograd);
 *     fabind_mul_dropmask_colsum, fabind_drop_mix (+ _bwd) added, fabind_gemm's fp32 (+ residual) epilogue takes p_drop (train-mode dropout
 *     ahead of a residual).
 * 18 = round 6: fabind_loss_fwd / fabind_loss_bwd / fabind_loss_blocks (the six-term training loss and its gradient seeds, one launch each way),
 *     fabind_pocket_center_fwd / _bwd (the Gumbel-softmax pocket centre, one launch each way); fabind_gemm_tn_set_exp ignores bit 2;
 *     fabind_pair_dist_fwd / _bwd, fabind_block_hadamard_bwd (+ fabind_pair_block_tile / _chunk): the distance head's pair operations on block descriptors;
 *     FabindGemmArgs.c2_bf16; fabind_node_chain_x3_fwd (node MLP / Transition as one split-precision kernel).
 *     Backward-compatible additions under 18: fabind_sym_automorphisms / fabind_sym_score (ligand automorphisms, symmetry-corrected RMSD).
 * 19 = fabind_las_step writes a per-node clamp mask (new argument pass_mask), fabind_las_step_bwd takes it in place of x_out: the adjoint's
 *     clamp decision is the forward's own (it used to be inferred from x_out - x, which fp32 rounding falsifies).
 *     Backward-compatible additions under 19: fabind_multi_sqnorm / fabind_multi_adam + FabindAdamRow, fabind_adam_chunk (the fused Adam / AdamW
 *     step with global-norm clip and non-finite skip; fabind_sizeof_args(5) = sizeof(FabindAdamRow)).  Purely additive: no existing entry
 *     point or struct changed, so the version stays.  Likewise fabind_gemm_plan + FB_GEMM_FAM_* (which kernel and epilogue fabind_gemm
 *     selects, reported without a launch).
 *     Likewise fabind_pose_stats / fabind_rank_loss_fwd (csrc/ranking.hip: FABind+ confidence training).
 *     Likewise fabind_pose_pair_rmsd / fabind_pose_cluster (csrc/pose_cluster.hip: the poses of a complex against each other, leader clustering).
 *     Likewise the form report of csrc/norm.hip (fabind_layernorm_rows_form, _rows_bwd_form, fabind_row_stats_form, fabind_edge_lnfold_form /
 *     _blocks, fabind_edge_lnfold_bwd_form, fabind_inter_coord_fold_blocks + FB_LNR_* / FB_LNB_* / FB_RST_* / FB_ELF_* / FB_ELB_*).
 *     Likewise fabind_torsion_plan / fabind_conformer_perturb (csrc/conformer.hip: train-time torsion noise and random rotation)
 *     and fabind_conformer_fit (csrc/conformer_fit.hip: the start conformer fitted to a pose in torsion space).
 *     Likewise fabind_las_pairs (csrc/topology.hip: LAS constraint pairs from the bond list).
 *     Likewise fabind_validity_plan / fabind_pose_check (csrc/pose_check.hip: physical validity of sampled poses).
 *     Likewise fabind_protein_grid / fabind_pose_protein_check (csrc/protein_contacts.hip: poses against all protein heavy atoms).
 *     Likewise fabind_pose_relax (csrc/pose_relax.hip: poses relaxed out of protein and internal clashes in torsion space).
 *     Likewise fabind_embed_bounds / fabind_embed_conformers (csrc/embed.hip: start conformers from the bond list by distance geometry).
 *     Likewise fabind_conformer_pair_rmsd / fabind_conformer_cross_rmsd (csrc/conformer_rmsd.hip: superposed symmetric RMSD of conformers).
 *     Likewise fabind_pose_score (csrc/pose_score.hip: a Vina-style intermolecular energy of sampled poses).
 * A binding must refuse a library whose version differs from the header it was written against. */
#define FABIND_ABI_VERSION 19
int fabind_abi_version(void);
/* sizeof() of an argument struct as this library was compiled: which = 0 FabindGemmArgs, 1 FabindEdgeBwdArgs,
 * 2 FabindPairUpdateArgs, 3 FabindTnJob, 4 FabindAttnFusedBwdArgs, 5 FabindAdamRow (-1 for an unknown index).  Lets a foreign-language mirror of the struct verify its layout. */
int fabind_sizeof_args(int which);

/* ---------------------------------------------------------------------------------------------
 * Dense contractions.  Replaces every nn.Linear / torch.cat+Linear / einsum+Linear on the path:
 * models/egnn.py:40-60,81,104,119,160-170,197-208; models/model_utils.py:83-92,103-131,168-174,
 * 196-222; models/model.py:100-101,117,132,139,358.
 *   C[M,N] = epi( pro(A|A2)[M,K] * W[N,K]^T )
 *   pro: act_pro applied to A while staging; columns [0,K1) come from A, [K1,K) from A2.
 *   epi: v = alpha*acc + bias[n]; v = act_epi(v); v *= d(act)/dx (dact_epi) at aux[m,n];
 *        v += R[r_index ? r_index[m] : m, n]; v += C_old (accumulate); C = v;
 *        dot_out[m, n_tile] = sum_n v * dotvec[n]   (n_tile = column block of 128)
 *   groups != NULL: ragged batched mode, blockIdx.z picks int32[8] {a_row0, M, w_row0, N, c_off_lo,
 *        c_off_hi, ldc, 0}; bias is indexed by w_row0 + n.
 * -------------------------------------------------------------------------------------------*/
typedef struct FabindGemmArgs {
    const void* A;
    const void* A2;
    const void* W;
    void* C;
    const float* bias;
    const void* R;
    const int* r_index;
    const float* dotvec;
    float* dot_out;
    const void* aux;
    const int* groups;
    void* C2; /* optional second output: act_epi'(pre-activation), same dtype/ld as C (saved for backward) */
    int M, N, K, K1;
    int lda, lda2, ldw, ldc, ldr, ldaux, dot_ld;
    int a_dtype, w_dtype, c_dtype, aux_dtype;
    int act_pro, act_epi, dact_epi;
    int accumulate;
    int store_preact; /* C receives the value BEFORE act_epi (row-dot still sees act_epi(v)) */
    int n_groups, max_m, max_n;
    int groups_ext; /* groups are int32[16] {M, N, K, lda, a_off lo/hi, w_off lo/hi, c_off lo/hi, ldc}: ragged A/W/C */
    int epi_fast; /* set by fabind_gemm itself: index of a specialised epilogue (0 = generic) */
    int k_splits; /* >1: split the K loop over k_splits work-groups; C must be fp32 [k_splits, M, N] partials */
    float alpha;
    float p_drop;       /* > 0: epilogue dropout (train / sampling mode): after bias + activation, before the residual, the value is
                           multiplied by keep/(1-p) with keep = [hash32(drop_seed + row*N + col) & 0xffff >= round(p*65536)] */
    unsigned drop_seed;
    /* optional LayerNorm fold (act_epi = relu writing a bf16 C, or relu + row-dot only; bf16 operands; K % 64 == 0): the accumulator of row r, column c becomes
       row_rs[r] * (acc - row_mu[r] * col_c[c]) before bias / activation -- i.e. LN(A) W^T evaluated as a GEMM on the
       UN-normalised A with W pre-scaled by the LN weight, col_c = its row sums, bias = W ln_b + b */
    const float* row_mu; const float* row_rs; const float* col_c;
    /* optional bf16 copy of an fp32 C (plain fp32 outputs with bias and/or residual only -- the residual-stream Linears): the
       epilogue writes C16[m, n] = bf16(C[m, n]) next to C, so the GEMMs that consume the result as an MFMA operand need no
       separate conversion pass over it */
    void* C16; int ldc16;
    /* != 0 with fp32 A and fp32 W: the contraction runs as split bf16 ("bf16x3": every operand element x = hi + lo with
       hi = bf16(x), lo = bf16(x - hi); three bf16 MFMAs per product term, fp32 accumulate; ~2^-17 relative operand error) instead
       of the exact fp32 MFMA.  The reference contracts in fp32 (egnn.py:68-144, model_utils.py:83-131). */
    int split3;
    /* dtype of R (FB_DT_F32 = 0: the default; FB_DT_BF16: a bf16 residual stream -- the FABind+ pair embedding, cross_att.py:41-46 --
       is added without a converted copy; row-contiguous 16-byte reads when C is bf16 with no activation, no r_index) */
    int r_dtype;
    int c2_bf16;       /* round 6: != 0: C2 (the stored activation derivative) is written as bf16 although C is fp32 (fp32 hidden layer for a
                          split-precision second Linear, bf16 derivative for the unchanged backward); C16 then carries bf16(act(pre)) */
} FabindGemmArgs;

int fabind_gemm(const FabindGemmArgs* args, hipStream_t stream);

/* Which kernel fabind_gemm would run for `args` under the current development knobs, without launching anything: the same host
 * function fabind_gemm itself dispatches through (same argument checks, same return code).
 *   family:   FB_GEMM_FAM_* below; -1 for an empty problem (nothing is launched)
 *   epi_fast: the specialised epilogue the launch asks for (0 = generic, 1-16, 20-25).  The nt and glds kernels always run the
 *             generic epilogue; forms 20-25 fall back to it inside the kernel when N, ldc or an address rules out 16-byte accesses
 *   cfg:      FB_GEMM_FAM_PIPE: the tile configuration after the split-K and small-M switches (fabind_gemm_set_config /
 *             fabind_gemm_set_small_m); FB_GEMM_FAM_X3 / _X3_PRO: the tile height in units of 64 rows; 0 elsewhere
 * Any of the three pointers may be NULL. */
#define FB_GEMM_FAM_NT_F32 0      /* gemm_nt_kernel<float, float>: fp32 A, fp32 W, exact fp32 MFMA */
#define FB_GEMM_FAM_NT_F32_BF16 1 /* gemm_nt_kernel<float, bf16>: fp32 A rounded to bf16 while staged */
#define FB_GEMM_FAM_NT_BF16 2     /* gemm_nt_kernel<bf16, bf16>: bf16 operands the LDS-DMA kernels cannot take (K % 64, act_pro, alignment) */
#define FB_GEMM_FAM_GLDS 3        /* gemm_bf16_glds_kernel: two-buffer LDS-DMA (fabind_gemm_set_config(0)) */
#define FB_GEMM_FAM_PIPE 4        /* gemm_bf16_pipe_kernel: the pipelined LDS-DMA ring, configuration in cfg */
#define FB_GEMM_FAM_X3 5          /* gemm_x3_kernel: split-bf16 contraction of fp32 operands */
#define FB_GEMM_FAM_X3_PRO 6      /* gemm_x3_kernel with the prologue activation compiled in */
#define FB_GEMM_FAM_PERSIST 7     /* gemm_bf16_persist_kernel (fabind_gemm_set_persistent; off by default) */
int fabind_gemm_plan(const FabindGemmArgs* args, int* family, int* epi_fast, int* cfg);

/* Weight-gradient contraction without transposes: C_part[s][m][n] = sum_{e in split s} Y[e,m] * X[e,n]
 * (bf16 row-major operands, fp32 partials [splits, M, N]; zero_page = >= 16 zero bytes in device memory).
 * with_colsum != 0 (no groups): every split's partial is [M * N + M] floats, the last M being sum_{e in split s} Y[e,m] -- the bias
 * gradient dY^T 1 of the Linear whose weight gradient dY^T X this is (reference: autograd of nn.Linear, e.g. model_utils.py:162-175),
 * so that ONE fabind_split_sum over M * N + M elements finishes both. */
int fabind_gemm_tn(const void* Y, int ldy, const void* X, int ldx, float* C_part, int M, int N, int E, int splits,
                   const void* zero_page, const int* groups, int n_groups, int with_colsum, hipStream_t stream);
/* groups (optional, splits == 1): int32[8] per group {y_off lo/hi (elements), ldy, M, x_row0, E, c_off lo/hi}. */

/* MANY weight-gradient contractions as ONE launch + ONE reduction launch.  Replaces the per-Linear `grad_weight = grad_output^T input`,
 * `grad_bias = grad_output^T 1` of torch autograd (nn.Linear at egnn.py:40-60,81,104,119,197-208, model_utils.py:83-131,162-175) for a
 * whole backward pass: the host queues the contractions as their operands become available and flushes the queue before the first
 * consumer of a result.  On a pocket-sized batch (9,000 nodes) one contraction is 32 work-groups of the 256-CU chip and the step has 89 of
 * them; together they fill it.
 * A job: out[m, n] (out_dt, row stride ldo) = sum_e Y[e, m] X[e, n]  and, with_colsum != 0, out_tail[m] (fp32) = sum_e Y[e, m]; bf16
 * row-major operands; C_part = this job's scratch of splits * (M * N + (with_colsum ? M : 0)) floats.  The contraction kernel is
 * fabind_gemm_tn's 256 x 256 layout: job j owns work-groups [wg0, wg0 + n_wg) with n_wg = n_tiles * roundup8(splits), wg0 a multiple of
 * 8 (the XCD-aware order of the single launch holds inside every job), n_tiles = ceil(M / 256) * ceil(N / 256),
 * e_per = roundup32(ceil(E / splits)); the reduction kernel gives job j blocks [blk0, blk0 + n_blk), n_blk = ceil((M * N (+ M)) / 4096).
 * jobs_dev / wg_job_dev (int32 job index per work-group) / blk_job_dev (per reduction block) are DEVICE tables, jobs_host the HOST copy
 * of the same jobs (validated here; the device cannot be read without synchronising). */
typedef struct FabindTnJob {
    const void* Y; const void* X; float* C_part; void* out; float* out_tail;
    int ldy, ldx, M, N, E, splits, e_per, n_tiles, with_colsum, out_dt, ldo;
    int wg0, n_wg, blk0, n_blk, pad_;
} FabindTnJob;
int fabind_gemm_tn_multi(const FabindTnJob* jobs_dev, const FabindTnJob* jobs_host, int n_jobs, const int* wg_job_dev, int total_wg,
                         const int* blk_job_dev, int total_blk, const void* zero_page, hipStream_t stream);

/* out[C,R] = act(in[R,C])^T -- feeds weight-gradient contractions (autograd of the ops above). */
int fabind_transpose_act(const void* in, int in_dt, int ldi, void* out, int out_dt, int ldo, int R, int C, int act,
                         hipStream_t stream);
/* Many strided 2-D copies with dtype conversion in one launch (the differentiable parameter pack of a model call -- slices,
 * concatenations, zero padding and casts of nn.Module parameters, models/*.py __init__ layouts -> kernel operand layouts -- and its
 * adjoint).  The table lives in DEVICE memory; strides are in elements; src == NULL writes zeros; vec4 != 0 promises column-contiguous,
 * 4-element-aligned rows on both sides with cols % 4 == 0. */
typedef struct FabindCopySeg {
    const void* src;
    void* dst;
    long long src_sr, src_sc, dst_sr, dst_sc;
    int rows, cols;
    int src_dt, dst_dt;
    int vec4, pad_;
} FabindCopySeg;
int fabind_multi_copy(const FabindCopySeg* segs_dev, int n_segs, int blocks_per_seg, hipStream_t stream);
/* Fused Adam / AdamW step over many fp32 tensors with the global-norm clip and a non-finite guard folded in: two launches per step.
 * Replaces torch.nn.utils.clip_grad_norm_ + torch.optim.Adam / AdamW.step() after backward (reference main_fabind.py:257-260, 419-426).
 * One DEVICE table of rows, one per tensor that has a gradient this step, sorted by chunk0: a tensor is cut into chunks of
 * fabind_adam_chunk() elements and row r owns chunks [chunk0[r], chunk0[r + 1]) of n_chunks (chunk0[0] = 0, numel >= 1).  All four
 * tensors are contiguous fp32 of numel elements, 4-byte aligned (16-byte accesses are used where the addresses allow; the result does
 * not depend on the alignment).  Hyper-parameters are doubles, as torch holds them; step_idx indexes the fp32 step-counter vector.
 *   fabind_multi_sqnorm: partials[c] = sum of g^2 over chunk c (fixed order, no atomics); snap[r] = steps[step_idx[r]].
 *   fabind_multi_adam:   total_norm = sqrt(sum_c partials[c]) (double, one fixed order in every block) -> *grad_norm;
 *       flags bit 0: g is scaled by min(1, max_norm / (total_norm + 1e-6)); bit 1: a non-finite total_norm skips the step (nothing of
 *       p / m / v / steps is written, *skipped += 1).  Otherwise torch 2.10's single-tensor Adam arithmetic with t = snap[r] + 1, and
 *       steps[step_idx[r]] = snap[r] + 1.  g is only read: the clip does not rescale it.
 * The two calls of a step share rows / n_rows / n_chunks / partials / snap and run in this order on one stream. */
typedef struct FabindAdamRow {
    float* p;
    const float* g;
    float* m;
    float* v;
    long long numel;
    int chunk0, step_idx;
    double lr, beta1, beta2, eps, weight_decay;
    int decoupled, pad_;
} FabindAdamRow;
int fabind_adam_chunk(void);
int fabind_multi_sqnorm(const FabindAdamRow* rows_dev, int n_rows, int n_chunks, const float* steps, float* partials, float* snap,
                        hipStream_t stream);
int fabind_multi_adam(const FabindAdamRow* rows_dev, int n_rows, int n_chunks, const float* partials, const float* snap, float* steps,
                      float max_norm, int flags, float* grad_norm, int* skipped, hipStream_t stream);
/* (round 6: src_dt = 2 = an fp32 source whose LO plane is packed, bf16(w - bf16(w)): with src_dt = 0 of the same source the hi | lo
 * fragment packs of the split-precision kernels.)
 * Many [N, K] weights (fp32 or bf16; element (n, k) at src[n * src_sr + k * src_sc], so a transposed source is a stride swap) into the
 * bf16 MFMA-fragment order [K/32][N/16][4][16][8] the fused edge / pair kernels take (fabind_gcl_edge_fused: W2p, Wcp; FabindEdgeBwdArgs:
 * W2p, Wcp, W2Tp, WcTp), one launch for all.  segs_dev: the table in DEVICE memory, segs_host: the same table on the host (validated). */
typedef struct FabindPackSeg {
    const void* src;
    void* dst;
    long long src_sr, src_sc;
    int N, K, src_dt, pad_;
} FabindPackSeg;
int fabind_pack_frag_multi(const FabindPackSeg* segs_dev, const FabindPackSeg* segs_host, int n_segs, hipStream_t stream);
/* out[i] = sum_s part[s * n + i] (fixed order), written as out_dt: the split reduction of fabind_gemm_tn / split-K partials. */
int fabind_split_sum(const float* part, int splits, long n, void* out, int out_dt, long n_tail, float* out_tail, hipStream_t stream);
/* n_tail > 0: the LAST n_tail of the n elements are written to out_tail as fp32 instead (a bias gradient behind a bf16 weight gradient). */
/* out[c] (+)= sum_r in[r,c]; scratch = float[nchunk*C] (bias gradients, deterministic two-pass). */
int fabind_colsum(const void* in, int in_dt, int ldi, float* out, int R, int C, int accumulate, float* scratch,
                  int nchunk, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Edge construction.  Replaces ComplexGraph.construct_edges + _radial_edges (models/att_model.py:
 * 37-128: dense [N,max_n] mask + nonzero) with direct row-sorted CSR emission.
 *   ctx graph  (row aggregates): ligand bonds (as given), protein-protein pairs with |xu-xv| <= cut_intra
 *              (normalised units), star edges to the segment's global node, glb_c<->glb_p.
 *   inter graph: ligand-atom <-> protein-residue pairs with |xu-xv| <= cut_inter, both directions.
 * count: fills deg_ctx[N], deg_int[N].  The caller scans them into rowptr (fabind_exclusive_scan).
 * fill : writes col / row (COO row per edge) arrays for both graphs.
 * bond_row/bond_col: ligand bonds (global node ids), complex-contiguous; bond_off[B+1] their ranges.
 * -------------------------------------------------------------------------------------------*/
int fabind_edges_count(const float* x, const int* node_off, const int* c_cnt, int B, int max_n, const int* bond_row,
                       const int* bond_off, float cut_intra, float cut_inter, int* deg_ctx, int* deg_int,
                       hipStream_t stream);
int fabind_edges_fill(const float* x, const int* node_off, const int* c_cnt, int B, int max_n, const int* bond_row,
                      const int* bond_col, const int* bond_off, float cut_intra, float cut_inter,
                      const int* rowptr_ctx, const int* rowptr_int, int* col_ctx, int* row_ctx, int* col_int,
                      int* row_int, hipStream_t stream);
/* out[0]=0, out[i+1]=out[i]+in[i], i<n (single work-group scan; n up to a few million). */
int fabind_exclusive_scan(const int* in, int* out, int n, hipStream_t stream);
/* out[k] = first index i with vals[i] >= keys[k] (n if none), vals non-decreasing int32 [n]: per-complex [start, end) offsets of a
 * complex-contiguous edge / bond / LAS list from node_off (keys = node_off [B + 1] gives out [B + 1]).  Replaces the bucketize +
 * histogram + cumsum index glue around att_model.py:37-116 / egnn.py:433-449's per-sample loops. */
int fabind_lower_bound(const int* vals, int n, const int* keys, int n_keys, int* out, hipStream_t stream);
/* Inter-edge pair bookkeeping (replaces trio_encoder's index arithmetic, models/egnn.py:286-304):
 * red_off[B+1] = prefix of ligand-row inter edges per complex; for every inter edge e, red_idx[e] =
 * index of its unordered (ligand, protein) pair in the reduced list; red_c/red_p = the pair's nodes;
 * mirror[e] = index of the reversed edge (the inter graph is symmetric). */
int fabind_inter_meta(const int* node_off, const int* c_cnt, int B, const int* rowptr_int, const int* col_int,
                      const int* row_int, int E_int, int* red_off, int* red_idx, int* red_c, int* red_p, int* mirror,
                      hipStream_t stream);
/* If the batch has no inter edge the reference inserts one fake symmetric pair (att_model.py:85-86);
 * host-side logic handles that case by calling fill with a forced pair -- see fabind_amd/graph.py. */

/* coord2radial with norm_type='per_sample' (models/egnn.py:767-787): d[e]=x[row]-x[col],
 * rho=|d|^2, rhohat = rho / sqrt(sum_{e in complex} rho^2).  Edges of a complex are contiguous:
 * [rowptr[node_off[b]], rowptr[node_off[b+1]]).  Also writes rho (un-normalised) and norm[b]. */
int fabind_edge_geom(const float* x, const int* row, const int* col, const int* rowptr, const int* node_off, int B,
                     float* d, float* rho, float* rhohat, float* norm, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * MC_E_GCL pieces (models/egnn.py:68-144).
 * gcl_pre:  pre[e,:] = act( AB[row[e], 0:H] + AB[col[e], H:2H] + rhohat[e]*w_r[:] )   (act = NONE keeps the
 *           pre-activation for training; SILU is the forward-only form)
 *           (first edge_mlp Linear split column-wise: node-level projections gathered per edge).
 * segment_sum: out[r,:] = sum_{e in row r} act(Z[eidx ? eidx[e] : e,:])   (unsorted_segment_sum on a row-sorted
 *           CSR; eidx = permutation for reductions over the column index, used by backward passes)
 *           n_edges = rowptr[n_rows] (host copy).  bf16 rows are reduced edge-balanced (64 CSR positions per wave,
 *           rows cut by a chunk boundary finish with fp32 atomics); fp32 rows one wave per row, fixed order.
 * coord_mean: x_out[r] = x[r] + clamp( (1/max(deg,1)) * sum_e d[e]*s[e], +-clampv ),
 *           s[e] = sum_k s_part[e,k] (row-dot partials written by fabind_gemm).
 * -------------------------------------------------------------------------------------------*/
int fabind_gcl_pre(const void* AB, int ab_dt, int ldab, int H, const int* row, const int* col, const float* rhohat,
                   const float* w_r, void* pre, int pre_dt, int E, int act, void* dact_out, hipStream_t stream);
int fabind_segment_sum(const void* Z, int z_dt, int ldz, int H, const int* rowptr, const int* eidx, int n_rows, int n_edges,
                       int act, float* out, int ldo,
                       void* out16 /* NULL, or a bf16 copy of the result [n_rows, ldo16]; `out` may then be NULL */, int ldo16,
                       hipStream_t stream);
/* out[r, 0:C) (and out2[r, 0:C), if given) = 0 for every row r of a CSR with no entries (rowptr[r] == rowptr[r+1]): the rows the fused
 * edge kernels' segment sums (egnn.py:84,790-821 unsorted_segment_sum) do not write. */
int fabind_zero_empty_rows(const int* rowptr, int n_rows, void* out, int out_dt, int ld, int C, void* out2, int out2_dt, int ld2,
                           hipStream_t stream);
int fabind_coord_update(const float* x, const float* d, const float* s_part, int n_part, const float* weight,
                        const int* rowptr, int n_rows, int mean, float clampv, float* x_out, float* s_out,
                        hipStream_t stream);

/* The same fused forward edge pipeline (models/egnn.py:68-128) in SPLIT-bf16 arithmetic (precision mode 'bf16x3': fp32-grade results
 * on the bf16 matrix cores, three MFMAs per product term): AB = fp32 [N, 2H]; every packed weight is given as TWO fragment arrays in
 * the layout of fabind_gcl_edge_fused, W..ph = bf16(W) and W..pl = bf16(W - float(W..ph)); agg / s_out / bnd / dropout as there.
 * n_rows = rows of AB (and of agg): n_rows * ldab * 4 bytes must stay below 4 GiB (32-bit gather offsets). */
int fabind_gcl_edge_fused_x3(const float* AB, int ldab, int n_rows, int H, const int* row, const int* col, const float* rhohat,
                             const float* w_r, const void* W2ph, const void* W2pl, const float* b2, const void* Wcph,
                             const void* Wcpl, const float* bc, const float* w3, int E, float* agg, float* s_out, float p_drop,
                             unsigned seed, float* bnd, hipStream_t stream);
/* The same for a 'bf16x3' training step (round 5): additionally leaves M [E, H] bf16 row-major (= bf16 of the split-precision messages),
 * d2f / z3f = silu'(pre2) x keep and pre3 as bf16 in accumulator-fragment order -- exactly what fabind_gcl_edge_fused_train leaves, so the
 * two-contraction backward (FabindEdgeBwdArgs.d2f / z3f, bf16 copy of AB) serves this mode too (reference arithmetic: egnn.py:68-128). */
int fabind_gcl_edge_fused_x3_train(const float* AB, int ldab, int n_rows, int H, const int* row, const int* col, const float* rhohat,
                                   const float* w_r, const void* W2ph, const void* W2pl, const float* b2, const void* Wcph,
                                   const void* Wcpl, const float* bc, const float* w3, int E, float* agg, float* s_out, float p_drop,
                                   unsigned seed, float* bnd, void* M, void* d2f, void* z3f, hipStream_t stream);

/* Fused forward edge pipeline of MC_E_GCL (models/egnn.py:68-128) for 64-edge tiles, bf16:
 *   s_out[e] = w3 . silu( silu( silu(A[row]+Bc[col]+rhohat*w_r) W2^T + b2 ) Wc^T + bc ),  agg[row] += silu(.. W2^T + b2)
 * AB = bf16 [N, 2H] (A | Bc); W2p / Wcp = bf16 weights packed in MFMA fragment order [H/32][H/16][4][16][8];
 * agg must be zero-initialised (nodes without edges are not written); every node with edges gets ONE plain store -- runs that
 * span 64-edge tiles are added in tile order by a fix-up kernel through `bnd`, so the sum is deterministic.  H in {64,128,256,512}.
 * p_drop > 0 (train mode, egnn.py:82): the messages are multiplied by keep(e,c)/(1-p) before both consumers, with
 *   keep(e,c) = [ half_{e&1}( hash32(seed + (e>>1)*H + c) ) >= round(p*65536) ],
 *   hash32(x): x^=x>>16; x*=0x7feb352d; x^=x>>15; x*=0x846ca68b; x^=x>>16   (evaluated again by the backward). */
int fabind_gcl_edge_fused(const void* AB, int ldab, int H, const int* row, const int* col, const float* rhohat,
                          const float* w_r, const void* W2p, const float* b2, const void* Wcp, const float* bc,
                          const float* w3, int E, float* agg, float* s_out, float p_drop, unsigned seed,
                          float* bnd /* scratch: ceil(E/64) x 2 x H floats (boundary runs of nodes that span tiles) */,
                          void* agg16 /* NULL, or [n_rows, H] bf16: the aggregated messages as the next contraction's operand */,
                          hipStream_t stream);

/* The same forward for a training step: additionally leaves M [E, H] bf16 row-major (the messages after dropout: operand of
 * d Wc = dT^T M), and d2f / z3f = silu'(pre2) x keep and pre3 = M Wc^T + bc as bf16 in the kernel's accumulator-fragment order
 * (ceil(E/64) x 64 x H elements each; opaque to the caller, consumed by fabind_gcl_edge_fused_bwd through FabindEdgeBwdArgs.d2f / z3f),
 * so that the backward chains two H x H contractions per edge instead of four (no forward recompute). */
int fabind_gcl_edge_fused_train(const void* AB, int ldab, int H, const int* row, const int* col, const float* rhohat,
                                const float* w_r, const void* W2p, const float* b2, const void* Wcp, const float* bc,
                                const float* w3, int E, float* agg, float* s_out, float p_drop, unsigned seed, float* bnd,
                                void* agg16, void* M, void* d2f, void* z3f, hipStream_t stream);

/* Backward of the fused edge pipeline (training, bf16): recomputes the forward per 64-edge tile and chains the four
 * H x H contractions of the adjoint (autograd of models/egnn.py:68-128).  Inputs: the forward's operands, ds [E]
 * (gradient of s), dagg [n_rows, lddagg] fp32 (gradient of agg); W2p/Wcp = fragment-packed W2 / Wc, W2Tp/WcTp =
 * fragment-packed W2^T / Wc^T.  Outputs: S1, Mm, dT, dP2 [E,H] bf16 = operands of the weight gradients
 * (dW2 = dP2^T S1, dWc = dT^T Mm via fabind_gemm_tn), dP1 [E,H] bf16 (gradient at the first Linear's output; the
 * caller reduces it over the sending node), drh [E], dABrow [n_rows, lddab] fp32 (zero-initialised by the caller:
 * receiving-side segment sum of dP1) and part [n_groups][4][H] fp32 partial column sums {d b2, d bc, d w3, d w_r}
 * (the caller adds the n_groups rows).  n_groups = number of persistent work-groups (<= number of CUs). */
typedef struct FabindEdgeBwdArgs {
    const void* AB; const int* row; const int* col; const float* rhohat; const float* w_r;
    const void* W2p; const void* Wcp; const void* W2Tp; const void* WcTp;
    const float* b2; const float* bc; const float* w3; const float* ds; const float* dagg;
    void* S1; void* Mm; void* dT; void* dP2; void* dP1;
    float* drh; float* dABrow; float* part;
    void* dbg;               /* NULL, or 12 x int64: cycle counts per phase of work-group 0 (profiling aid; two-tile variant) */
    float* bnd;              /* ceil(E / tile) x 2 x H floats of scratch (boundary runs of dABrow, added in tile order: deterministic) */
    void* d2scratch;         /* single-tile variant: n_groups x 64 x H x 2 bytes of scratch (silu'(pre2) of each work-group's tile) */
    int ldab, lddagg, lddab, E;
    float p_drop;            /* dropout probability of the messages (egnn.py:82); 0 = eval */
    unsigned seed;           /* the seed the forward call used */
    int xcd_aware;           /* filled in by the library (fabind_gcl_edge_fused_set_xcd_aware); callers pass 0 */
    int lddab16;
    void* dAB16;             /* NULL, or [N, lddab16] bf16: the receiving-side sums go to its columns [0, H) INSTEAD of dABrow (variant 5
                              * only; the caller reduces dP1 into columns [H, 2H) with fabind_segment_sum's out16) */
    const void* d2f;         /* NULL, or silu'(pre2) as saved by fabind_gcl_edge_fused_train (bf16, ceil(E/64) x 64 x H, fragment order) and */
    const void* z3f;         /* pre3 likewise: the launch then takes the TWO-contraction kernel (csrc/fused_edge_bwd4.hip), which reads these
                              * instead of recomputing them, does NOT write Mm (the forward's M is the weight gradient's operand) and needs
                              * neither d2scratch nor dbg; n_groups up to 2 x CUs at H = 512 (64 KiB LDS tile, <= 128 VGPRs) */
} FabindEdgeBwdArgs;
int fabind_gcl_edge_fused_bwd(const FabindEdgeBwdArgs* args, int H, int n_groups, hipStream_t stream);
/* Edges per tile of the backward kernel: 64 (one work-group per CU, default) or 32 (two per CU). */
int fabind_gcl_edge_fused_bwd_set_tile(int bm);
int fabind_gcl_edge_fused_bwd_tile(void);
/* Kernel variant: 0 (default) = two [64][H] LDS tiles, one work-group per CU; 1 = ONE LDS tile rewritten in place by every stage,
 * two work-groups per CU so that one work-group's elementwise epilogue can overlap the other's contraction (needs
 * FabindEdgeBwdArgs.d2scratch; n_groups up to 2 x CUs) -- measured no faster, kept as a knob.  Both
 * evaluate the same arithmetic in the same order per element (outputs equal to 1e-7). */
int fabind_gcl_edge_fused_bwd_set_variant(int v);
int fabind_gcl_edge_fused_bwd_variant(void);
int fabind_gcl_edge_fused_bwd_variant_for(int H);   /* the variant a launch at hidden size H takes: the set one, or -- when none was set explicitly -- 0 for H <= 128 (measured faster there), 5 otherwise.  The caller sizes d2scratch / n_groups from THIS value */
/* development knob of variants 3 / 4: bit mask of work the kernel SKIPS (results are then wrong -- sensitivity timing only). */
void fabind_gcl_edge_fused_bwd3_set_exp(int mask);
void fabind_gcl_edge_fused_bwd4_set_exp(int mask);   /* the saved-forward kernel: 1 dT / dP2 copy-outs, 2 S1 / dP1 stores, 4 row scan, 8 both contractions */
/* development knob: 1 (default) = XCD-aware tile order in the fused edge kernels (XCD x owns the x-th eighth of the tiles, i.e.
 * whole complexes); 0 = linear tile order (forward) / grid-stride walk (backward).  Results do not depend on it. */
void fabind_gcl_edge_fused_set_xcd_aware(int on);
/* Forward kernel variant: 1 (default) = row-wise gather + operand-swapped epilogues (csrc/fused_edge_fwd2.hip), 0 = round 1's kernel. */
int fabind_gcl_edge_fused_set_variant(int v);
int fabind_gcl_edge_fused_variant(void);

/* Fused pair-embedding update of FABind+'s CrossAttentionModule (FABind_plus/fabind/models/cross_att.py:42-44 with
 * model_utils.py InteractionModule / MLPwithLastAct), bf16, inference (no adjoint: training runs the separate launches):
 *   z1 = z_in + (T[p_node, 0:32] * T[c_node, b_off:b_off+32]) Wo^T + bo;   y = LayerNorm(z1; ln_w, ln_b, eps)
 *   z_out = drop(relu( drop(relu(y W1^T + b1)) W2^T + b2 ));   bias_out = z_out Wb^T + bb   (when Wbp != NULL)
 * z_in / z_out: bf16 [n_pairs, H] (may alias); T: fp32 [nodes, ldt]; p_node / c_node: int32 [n_pairs].
 * Wop = [H,32], W1p / W2p = [H,H], Wbp = [16,H], all bf16 packed in MFMA fragment order [K/32][N/16][4][16][8].
 * Dropout (sampling mode): keep(e,c) of fabind_gcl_edge_fused with seed (first) and seed + 0x9e3779b9 (second). */
typedef struct FabindPairUpdateArgs {
    const float* T; const int* p_node; const int* c_node;
    const void* z_in; void* z_out;
    const void* Wop; const float* bo; const float* ln_w; const float* ln_b;
    const void* W1p; const float* b1; const void* W2p; const float* b2;
    const void* Wbp; const float* bb; float* bias_out;
    int ldt, b_off, n_pairs;
    float eps, p_drop;
    unsigned seed;
} FabindPairUpdateArgs;
int fabind_pair_update_fused(const FabindPairUpdateArgs* args, int H, hipStream_t stream);

/* Ligand post-optimisation (FABind/fabind/utils/post_optim_utils.py:9-64; called per complex by fabind_inference.py:285-328):
 * `steps` Adam iterations (lr, betas 0.9 / 0.999, eps 1e-8) on x0 against
 *   sum_{(i,j) in LAS} | |x_i-x_j| - |ref_i-ref_j| | + 2 sum_{i,j} relu(1.22 - |x_i-x_j|)      (all_pairs = 0), or
 *   sum_{i,j} | |x_i-x_j| - |ref_i-ref_j| |                                                  (all_pairs = 1: no LAS edges)
 * for a BATCH of ligands in one launch (one work-group per ligand, all iterations inside the kernel).
 * x0, ref, x_out: fp32 [sum atoms, 3]; atom_off: int32 [n_ligands+1]; nbr_ptr int32 [sum atoms + 1] / nbr_idx int32 (GLOBAL
 * atom ids): for every DISTINCT directed LAS edge (i,j) the list of i holds j and the list of j holds i.
 * loss_out[l] = loss at the last iteration (before its step), rmsd_out[l] = sqrt(mean |ref - x_out|^2), like the reference's
 * return values.  max_atoms = largest ligand (<= 512). */
int fabind_post_optimize(const float* x0, const float* ref, const int* atom_off, const int* nbr_ptr, const int* nbr_idx,
                         int n_ligands, int max_atoms, int all_pairs, int steps, float lr, float* x_out, float* loss_out,
                         float* rmsd_out, hipStream_t stream);

/* Ligand poses from a predicted distance map (FABind/fabind/utils/generation_utils.py:42-120): `epochs` Adam iterations (lr, betas
 * 0.9 / 0.999, eps 1e-8) on the start coordinates x0 of n_repeat starts of a BATCH of ligands in one launch (one work-group per
 * (ligand, repeat), all epochs inside the kernel).  With dis = min(|p_i - x_k|, 10) and r = dis - y_pred[i, k], at 0-based epoch t
 *   interaction   = sum |r| (mode 0) | sum r^2 (mode 1) | sum (|r| + 1e-5)^0.5 (mode 2)
 *   configuration = sum over the listed ordered pairs (k,j) of | |x_k-x_j| - D_kj |  + (excluded_volume ? 2 sum_{k,j} relu(1.22 - |x_k-x_j|) : 0)
 *   loss          = interaction (t < config_start), else interaction + config_rate (t - config_start) configuration.
 * x0, x_out: fp32 [n_repeat, n_atoms, 3]; truth fp32 [n_atoms, 3] (the pose the RMSD is taken to); atom_off int32 [n_ligands + 1];
 * pocket fp32 [sum residues, 3] with pocket_off int32 [n_ligands + 1]; y_pred fp32 flat, ligand l at y_off[l] (int64 [n_ligands]) as
 * [residues_l, atoms_l] with the atom index fastest (the layout of the model's distance head).  con_ptr int32 [n_atoms + 1] /
 * con_idx int32 (GLOBAL atom ids) / con_d fp32: for every listed ordered pair (k,j) the list of k holds (j, D_kj) and the list of j
 * holds (k, D_kj); each entry weighs 1/2 in the loss and 1 in its owner's gradient.
 * loss_out / rmsd_out fp32 [n_repeat, n_ligands], terms_out fp32 [n_repeat, n_ligands, 2] = (interaction, configuration): the loss of
 * the LAST epoch before its step, the RMSD after the last step.  trace_loss / trace_rmsd (both or neither, may be NULL): fp32
 * [n_repeat, n_ligands, epochs], every epoch's loss and RMSD.
 * max_atoms <= 512, max_pocket <= 4096 (largest ligand / pocket of the batch); max_con = most list entries of one ligand, max_y =
 * largest residues_l * (atoms_l | 1): both only decide whether the lists and y_pred are kept in LDS (144 KiB budget) or read from memory.
 * rate_lr: HOST pointer to two doubles, {config_rate, lr} (read before the call returns): the schedule weight and Adam's bias-corrected
 * step are formed in double from them, as torch forms them from python floats.  Modes 0 / 1 iterate in float, mode 2 in double.
 * Fixed-order sums, no atomics: a ligand's result does not depend on the batch or on n_repeat, and is bit-reproducible.
 * Backward-compatible addition under ABI 19. */
int fabind_distmap_generate(const float* x0, const float* truth, const float* pocket, const int* pocket_off, const float* y_pred,
                            const long long* y_off, const int* atom_off, const int* con_ptr, const int* con_idx, const float* con_d,
                            int n_ligands, int n_repeat, int n_atoms, int max_atoms, int max_pocket, int max_con, long max_y,
                            int excluded_volume, int mode, int epochs, int config_start, const double* rate_lr, float* x_out,
                            float* loss_out, float* terms_out, float* rmsd_out, float* trace_loss, float* trace_rmsd,
                            hipStream_t stream);

/* Ligand automorphisms (FABind_plus/fabind/utils/isomorphism.py:23-72: graph-tool subgraph_isomorphism(G, G, vertex_label=atomGetnum,
 * subgraph=False), run per molecule offline by tools/inject_isomorphism_to_data.py) for a BATCH of ligands, one wave per ligand.
 * labels: int32 [sum atoms]; nbr_ptr int32 [sum atoms + 1] / nbr_idx int32 (GLOBAL atom ids): symmetrised bond lists (every bond
 * (i,j) listed under i and under j; entries outside the ligand and self-loops are ignored); atom_off int32 [n_ligands + 1].
 * An automorphism a (int32 [n], a permutation) has label[a[i]] == label[i] and (i,j) bonded <=> (a[i],a[j]) bonded.
 * Count mode (scratch = flat = NULL): count[b] = number of automorphisms, stopping at cap + 1.  Write mode: flat_off int32
 * [n_ligands + 1] (element offsets; slot b holds min(count, cap) * n_b entries as count mode reported them), scratch / flat
 * int32 [flat_off[n_ligands]]; flat receives the automorphisms of each ligand in ascending lexicographic order (identity first),
 * count[b] = how many.  The identity is always kept; a truncated set is the identity plus the first cap - 1 others in search order.
 * status[b]: 0 ok, 1 more than cap automorphisms, 2 max_steps candidate assignments exhausted, 3 n_b > 256 (identity only).
 * Deterministic: integer arithmetic only. */
int fabind_sym_automorphisms(const int* labels, const int* nbr_ptr, const int* nbr_idx, const int* atom_off, int n_ligands, int cap,
                             int max_steps, const int* flat_off, int* scratch, int* flat, int* count, int* status, hipStream_t stream);
/* Minimum over a ligand's automorphisms (FABind_plus/fabind/utils/get_sym_rmsd.py:5-18 -- spyrmsd symmrmsd without centring or
 * superposition, per complex on the host in utils/training.py:273-286; utils/permutation_loss.py:4-33 -- the per-ligand argmin of
 * the mean Smooth-L1) for n_pose poses at once, one work-group per (ligand, pose):
 *   rmsd_k = sqrt(mean_i |pred[s, off_b + a_k[i]] - ref[off_b + i]|^2),  sl1_k = mean over the 3 n_b elements of SmoothL1 (beta 1).
 * pred fp32 [n_pose, n_atoms, 3], ref fp32 [n_atoms, 3]; flat / flat_off as written by fabind_sym_automorphisms; auto_cnt[b] =
 * automorphisms to use (0 = the identity alone: plain RMSD).  min_rmsd / min_sl1 fp32, arg_rmsd / arg_sl1 int32 [n_pose, n_ligands]:
 * the minimum and the FIRST k reaching it.  best_idx (optional, int32 [n_atoms]): off_b + a_k[i] for the Smooth-L1 argmin of pose 0
 * (the new_idx of the permutation-invariant loss).  Fixed summation order, no atomics: bit-reproducible.  max_atoms <= 2048. */
int fabind_sym_score(const float* pred, int n_pose, int n_atoms, const float* ref, const int* atom_off, const int* flat_off,
                     const int* auto_cnt, const int* flat, int n_ligands, int max_atoms, float* min_rmsd, int* arg_rmsd, float* min_sl1,
                     int* arg_sl1, int* best_idx, hipStream_t stream);
/* Train-time ligand augmentation (FABind_plus/fabind/utils/utils.py:155-190 get_torsions, :285-304 torsion noise, :45-81 / :307-311
 * uniform_random_rotation) for a BATCH of ligands.
 * fabind_torsion_plan: the rotatable bonds of every ligand and the atoms each one moves.  nbr_ptr int32 [sum atoms + 1] / nbr_idx
 *   (GLOBAL atom ids) / nbr_code / nbr_own int32 [n_entries]: the symmetrised, de-duplicated neighbour lists, sorted by owner and then
 *   by neighbour, with the bond code of every entry (AROMATIC 1, TRIPLE 2, DOUBLE 3, SINGLE 4, other 5) and its owner atom;
 *   atom_off int32 [n_ligands + 1].  j-k (j < k) is rotatable iff its code is SINGLE, j and k have heavy-atom degree >= 2, neither has
 *   a TRIPLE bond and the bond is on no cycle (the SMARTS [!$(*#*)&!D1]-&!@[!$(*#*)&!D1] on the heavy-atom graph).
 *   Count mode (quad = NULL): flag int32 [n_entries], scratch_quad int32 [4 n_entries], scratch_side uint32 [8 n_entries] are written
 *   per entry; count[b] = rotatable bonds of ligand b; status[b] = 0, or 3 for a ligand of more than 256 atoms (zero torsions).
 *   Write mode (the same flag / scratch buffers, tor_off int32 [n_ligands + 1] = exclusive sums of count): ligand b's torsions in
 *   ascending (j, k) order at [tor_off[b], tor_off[b + 1]): quad[t] = (i, j, k, l) local atom ids, i / l the lowest-index neighbour of
 *   j other than k / of k other than j; side[t] = eight 32-bit words, bit a of the 256-bit set <=> atom a is in k's component once
 *   j-k is removed.  Integer arithmetic only.
 * fabind_conformer_perturb: out fp32 [n_copies, n_atoms, 3] = n_copies perturbed images of x fp32 [n_atoms, 3]; one wave per (ligand,
 *   copy).  The torsions of the plan (tor_off / quad / side; tor_off = NULL: none) are set one after another to their targets (rotation
 *   of `side` about j -> k by target - current dihedral; by target itself when `relative`; a degenerate dihedral counts as 0), then,
 *   with `rotate`, the rotation M = -(H R) of uniform_random_rotation: out = (x - mean) M + mean M, without the last term (centroid at
 *   the origin) when `centre`.  Targets: angles fp32 [n_copies, t_total] (radians) or, angles = NULL, 2 pi u; (x1, x2, x3):
 *   uniforms fp32 [n_copies, n_ligands, 3] or, NULL, drawn; u(seed, key, copy, draw) is a counter-based hash of its four arguments
 *   (keys int32 [n_ligands]; NULL = the ligand's position), draws 0 .. T_b - 1 the torsions, then x2, x3, x1.  Fixed summation order:
 *   bit-reproducible.  Ligands of more than 256 atoms are rotated only. */
int fabind_torsion_plan(const int* nbr_ptr, const int* nbr_idx, const int* nbr_code, const int* nbr_own, const int* atom_off,
                        int n_ligands, int n_entries, int* flag, int* scratch_quad, unsigned* scratch_side, int* count, int* status,
                        const int* tor_off, int* quad, unsigned* side, hipStream_t stream);
int fabind_conformer_perturb(const float* x, const int* atom_off, int n_ligands, int n_atoms, int n_copies, const int* tor_off,
                             const int* quad, const unsigned* side, const float* angles, int t_total, const float* uniforms,
                             const int* keys, unsigned seed, int relative, int rotate, int centre, float* out, hipStream_t stream);
/* fabind_conformer_fit (csrc/conformer_fit.hip; a backward-compatible addition under ABI 19): the inverse of fabind_conformer_perturb.
 *   For every ligand b and every pose s of target fp32 [n_poses, n_atoms, 3]: the angles a of the ligand's torsions (tor_off / quad /
 *   side as fabind_torsion_plan writes them; tor_off = NULL: none) and the rigid motion for which pose(a) -- the torsions applied to
 *   x0 fp32 [n_atoms, 3] one after another as relative rotations, the rule of fabind_conformer_perturb, then the optimal proper
 *   rotation and translation onto the target (Horn's quaternion method in double) -- is closest to the target atom by atom:
 *   damped Gauss-Newton on E(a) = sum |pose(a) - y|^2 over the T_b torsions and six rigid components (normal matrix and Cholesky in
 *   double), lam from 1e-3, / 10 (floor 1e-9) after an accepted trial (E fell), * 10 after a rejected one.
 *   coords fp32 [n_poses, n_atoms, 3] = the fitted pose; angles fp32 [n_poses, t_total] in (-pi, pi], plan order (0 for a ligand
 *   fitted rigidly only); rmsd0 / rmsd fp32 [n_poses, n_ligands] = sqrt(E / n_b) after the rigid fit alone / at the end; iters int32
 *   = accepted steps; stop int32 = 0 (an accepted step lowered E by no more than tol E; also: nothing to iterate), 1 (max_iters
 *   accepted steps), 2 (8 rejections in a row); status int32 [n_ligands] = 0, 3 (more than min(max_atoms, 256) atoms) or 4 (more
 *   than min(max_torsions, 58) torsions): such a ligand gets the rigid fit only; trace (optional) fp64 [n_poses, n_ligands,
 *   max_iters] = E after each accepted step, NaN behind the last.  A ligand without atoms writes rmsd 0, iters 0.
 *   max_atoms / max_torsions (the largest n_b / T_b of the batch, or more) size the work-group's LDS.  One wave per (ligand, pose),
 *   one launch; every sum in an order fixed by the ligand alone, no atomics: the same bits alone, in any batch, among any poses. */
int fabind_conformer_fit(const float* x0, const float* target, const int* atom_off, int n_ligands, int n_atoms, int n_poses,
                         const int* tor_off, const int* quad, const unsigned* side, int t_total, int max_atoms, int max_torsions,
                         int max_iters, float tol, float* coords, float* angles, float* rmsd0, float* rmsd, int* iters, int* stop,
                         int* status, double* trace, hipStream_t stream);
/* LAS ("local atomic structure") constraint pairs of a BATCH of ligands from their bond lists (FABind/fabind/utils/generation_utils.py:
 * 170-187 get_LAS_distance_constraint_mask).  nbr_ptr int32 [sum atoms + 1] / nbr_idx int32 [n_entries] (GLOBAL atom ids): the
 * symmetrised, de-duplicated neighbour lists without self-loops, sorted by owner and then by neighbour; atom_off int32 [n_ligands + 1].
 * Pair (i, j), i != j, of one ligand is kept iff i and j are bonded, have a common neighbour, or lie on a common relevant cycle (a
 * cycle whose edge set is no GF(2) sum of strictly shorter cycles).
 *   Count mode (edge_index = NULL): row_count int32 [sum atoms] = pairs of every atom's row; mask_rows uint32 [sum atoms, 8] = the
 *   256-bit row of every atom of a ligand of at most 256 atoms (bit j of word j / 32); ring_pairs int32 [n_ligands] = unordered pairs
 *   on a common relevant cycle; status int32 [n_ligands] = 0, 3 (more than 256 atoms) or 4 (more than 64 non-tree bonds): such a ligand
 *   gets the bonded and common-neighbour pairs only.
 *   Write mode (the same mask_rows; row_off int32 [sum atoms + 1] = exclusive sums of row_count, n_pairs = row_off[sum atoms]):
 *   edge_index int64 [2, n_pairs], GLOBAL atom ids, row i's pairs at [row_off[i], row_off[i + 1]) in ascending j -- ligand by ligand,
 *   row-major: the order of dense_to_sparse.  Nothing is written at or beyond n_pairs.  Integer arithmetic only, no atomics. */
int fabind_las_pairs(const int* nbr_ptr, const int* nbr_idx, const int* atom_off, int n_ligands, int n_entries, int* row_count,
                     unsigned* mask_rows, int* ring_pairs, int* status, const int* row_off, long n_pairs, long long* edge_index,
                     hipStream_t stream);
/* FABind+ confidence training (FABind_plus/fabind/utils/training_confidence.py:41-77, :215-252).
 * fabind_pose_stats: per sample b over the atoms [atom_off[b], atom_off[b + 1]) (atom_off int32 [B + 1]; pred / truth fp32 [n_atoms, 3]):
 *   rmsd[b] = sqrt(mean_i |p_i - t_i|^2), cdis[b] = |mean_i (p_i - t_i)| (the distance of the two centroids); an empty sample gives
 *   0 / 0.  One wave per sample, fixed summation order.
 * fabind_rank_loss_fwd: the pairwise ranking loss of G groups of samples, group g = [group_off[g], group_off[g + 1]) (int32 [G + 1],
 *   2 <= size S <= 1024: the caller checks; a group outside that range gets NaN terms and zero counts).  b is better than a when
 *   (rmsd_b, b) < (rmsd_a, a); over the P = S(S-1)/2 pairs, delta = s_better - s_worse:
 *     mode 0 (logsigmoid)    term = max(-delta, 0) + log1p(exp(-|delta|))
 *     mode 1 (dynamic_hinge) term = relu((rmsd_worse - rmsd_better) - delta)
 *   ranking = sum / P; ce = mean_a BCE-with-logits(s_a, [rmsd_a < 2]) if with_ce else 0.
 *   terms fp32 [G, 3] = (ranking, ce, ranking + ce); d_scores fp32 [n_samples] = d (ranking + ce) / d s_a (relu' = 0 at 0);
 *   counts int32 [G, 4] = (#pairs with s_better > s_worse, P, [score of the best sample > every other score],
 *   #{a : [s_first > 0] == [rmsd_a < 2]} with s_first the group's first sample, as the reference's line 77 computes it).
 *   One work-group per group; fixed-order sums, no atomics, no state between launches: bit-reproducible.
 * Backward-compatible additions under ABI 19. */
int fabind_pose_stats(const float* pred, const float* truth, const int* atom_off, int B, float* rmsd, float* cdis, hipStream_t stream);
int fabind_rank_loss_fwd(const float* scores, const float* rmsd, const int* group_off, int G, int mode, int with_ce, float* terms,
                         float* d_scores, int* counts, hipStream_t stream);
/* The sampled poses of every complex against each other (csrc/pose_cluster.hip).  Backward-compatible additions under ABI 19.
 * fabind_pose_pair_rmsd: D fp32 [n_ligands, n_pose, n_pose],
 *   D[b, s, t] = min over the automorphisms a of ligand b of sqrt((1 / n_b) sum_i |x_s[off_b + a[i]] - x_t[off_b + i]|^2)
 *   (no centring, no superposition: the definition of fabind_sym_score) for poses fp32 [n_pose, n_atoms, 3]; atom_off, flat_off,
 *   auto_cnt, flat as fabind_sym_score takes them (auto_cnt[b] = 0: the identity alone, plain RMSD; never more entries than the
 *   ligand's slot of flat holds; an entry outside [0, n_b) counts as i).  Every unordered pair is computed once and written to both
 *   triangles (D is exactly symmetric), the diagonal is +0.0, a ligand without atoms gets 0.  The sum of a pair is formed in an order
 *   fixed by the ligand alone and minima are taken on bit patterns: D[b, s, t] is the same bits in any batch and among any n_pose
 *   poses.  No float atomics.  n_pose <= 512 and max_atoms (>= every n_b) <= 2048, refused otherwise before anything is launched.
 * fabind_pose_cluster: leader clustering of every ligand's poses on D with conf fp32 [n_pose, n_ligands]: rank by descending confidence
 *   (equal values in pose order, NaN last); the best unassigned pose leads the next cluster, every unassigned t with
 *   D[b, leader, t] < threshold (strict; a NaN distance never joins) joins it.  int32 outputs: cluster_id [n_pose, n_ligands] (0 = the
 *   cluster of the most confident pose); leader / size [n_pose, n_ligands]: row k = cluster k's leading pose and population, -1 / 0
 *   from row n_clusters[b] on; n_clusters [n_ligands].  One wave per ligand, comparisons and integers only.  n_pose <= 512. */
int fabind_pose_pair_rmsd(const float* poses, int n_pose, int n_atoms, const int* atom_off, const int* flat_off, const int* auto_cnt,
                          const int* flat, int n_ligands, int max_atoms, float* D, hipStream_t stream);
int fabind_pose_cluster(const float* D, const float* conf, int n_pose, int n_ligands, float threshold, int* cluster_id, int* leader,
                        int* size, int* n_clusters, hipStream_t stream);
/* Physical validity of sampled poses (csrc/pose_check.hip; fabind_amd/validity.py documents every layout).  Backward-compatible
 * additions under ABI 19.
 * fabind_validity_plan: the per-ligand plan from the coded neighbour lists of fabind_torsion_plan (nbr_ptr / nbr_idx / nbr_code, GLOBAL
 *   ids, sorted by owner and neighbour), atomic numbers z int32 [sum atoms] and the start conformer x0 fp32 [sum atoms, 3]; radii_in fp32
 *   [sum atoms] or NULL (Bondi radii by atomic number); auto_flat / auto_off / auto_cnt as fabind_sym_score takes them, or NULL.
 *   Count mode (offs = NULL): counts int32 [n_ligands, 4] = (ratio pairs, planar groups, group atoms, stereo centres), status int32
 *   [n_ligands] = 0, 3 (more than 256 atoms) or 5 (a bonded or 1-3 pair at distance 0 in x0): a ligand with status != 0 has no entries.
 *   Write mode (offs int32 [4, n_ligands + 1] = the exclusive sums of the four counts; status as the count pass left it): cls uint32
 *   [sum atoms, 16], two bits per pair (i, j) at bit 2 (j % 16) of word j / 16 of row i: 1 bonded, 2 angle, 3 clash, 0 exempt (the
 *   caller zeroes it); radii fp32 [sum atoms]; pair_ij int32 [pairs, 2] (local i < j, ascending), pair_kind int32 [pairs] (1 / 2),
 *   pair_d0 fp64 [pairs]; group int32 [groups, 3] = (0 aromatic / 1 double bond, first position in the ligand's slot of gatoms, atoms);
 *   gatoms int32 [group atoms] local ids; centre int32 [centres, 5] = (c, n1, n2, n3, n4 or -1); centre_v0 fp64 [centres].  A ligand
 *   whose counts differ from its slots writes no list.  One work-group per ligand, integer work in LDS, no atomics.
 * fabind_pose_check: stats fp32 [n_ligands, n_pose, 9] = (bond_lo, bond_hi, angle_lo, angle_hi, clash, flat_aromatic, flat_double,
 *   chirality, ca_dist) and flags int32 [n_ligands, n_pose] (1 BOND, 2 ANGLE, 4 CLASH, 8 AROMATIC_FLAT, 16 DOUBLE_FLAT, 32 CHIRALITY,
 *   64 PROTEIN, 128 NONFINITE, 256 UNCHECKED) of poses fp32 [n_pose, n_atoms, 3] under the plan; pocket fp32 [residues, 3] with
 *   pocket_off int32 [n_ligands + 1], or NULL; max_atoms >= every ligand of status 0, <= 256.  One wave per (ligand, pose), one launch
 *   whatever n_pose; float64 arithmetic on the float32 inputs; an entry is the same bits alone, in any batch and among any n_pose. */
int fabind_validity_plan(const int* nbr_ptr, const int* nbr_idx, const int* nbr_code, const int* atom_off, int n_ligands,
                         const int* z, const float* x0, const float* radii_in, float min_volume, const int* auto_flat,
                         const int* auto_off, const int* auto_cnt, int* counts, int* status, const int* offs, unsigned* cls,
                         float* radii, int* pair_ij, int* pair_kind, double* pair_d0, int* group, int* gatoms, int* centre,
                         double* centre_v0, hipStream_t stream);
int fabind_pose_check(const float* poses, int n_pose, int n_atoms, const int* atom_off, int n_ligands, int max_atoms,
                      const int* status, const unsigned* cls, const float* radii, const int* offs, const int* pair_ij,
                      const int* pair_kind, const double* pair_d0, const int* group, const int* gatoms, const int* centre,
                      const double* centre_v0, const float* pocket, const int* pocket_off, float bond_lo, float bond_hi,
                      float angle_lo, float angle_hi, float clash_min, float flat_max, float ca_min, int use_ca, float* stats,
                      int* flags, hipStream_t stream);
/* Sampled poses against all heavy atoms of the protein (csrc/protein_contacts.hip; fabind_amd/validity.py documents every layout).
 * Backward-compatible additions under ABI 19.
 * fabind_protein_grid: a cell list per complex of prot_xyz fp32 [sum atoms, 3], prot_z int32 [sum atoms], prot_off int32
 *   [n_complex + 1]; radii_in fp32 [sum atoms] or NULL (Bondi radii by atomic number).  The cell of an atom along an axis is
 *   floor(double(x) / double(edge)) clamped to +-2^29; atoms with z <= 1 are dropped.
 *   Count mode (cell_off = NULL): origin int32 [n_complex, 3] (lowest cell), dims int32 [n_complex, 3], status int32 [n_complex] = 0,
 *   6 (a non-finite coordinate) or 7 (a box of more than 2^20 cells), counts int32 [n_complex, 2] = (cells, kept atoms); a complex with
 *   status != 0 has origin = dims = 0 and no entries.
 *   Write mode (cell_off / kept_off int32 [n_complex + 1] = the exclusive sums of the two counts, n_cells / n_kept their totals; origin,
 *   dims and status as the count pass left them): cell_ptr int32 [n_cells + 1], positions into the sorted atoms; xyz fp32 [n_kept, 3],
 *   radii fp32 [n_kept], atom_id int32 [n_kept] (the id within the complex), ordered by (complex, cell, id).  Scratch: cell_of int32
 *   [sum atoms], cell_fill int32 [n_cells], slot int32 [n_kept].  Integer atomics build the histogram and fill the cells; the order
 *   within a cell is by id whatever the scheduling.
 * fabind_pose_protein_check: stats fp32 [n_complex, n_pose, 3] = (prot_clash, prot_dist, overlap), counts int32 [n_complex, n_pose, 3] =
 *   (n_close, n_lig, n_both), pair int32 [n_complex, n_pose, 2] = (ligand atom, protein atom) of the prot_clash minimum or (-1, -1),
 *   flags int32 [n_complex, n_pose] (1 PROTEIN_CLASH, 2 PROTEIN_OVERLAP, 128 NONFINITE, 256 UNCHECKED) of poses fp32 [n_pose, n_atoms, 3]
 *   of the ligands atom_off int32 [n_complex + 1] with radii lig_radii fp32 [n_atoms] and status plan_status (fabind_validity_plan)
 *   against the grid; max_atoms >= every ligand of status 0, <= 256; max_radius >= every protein radius, cutoff <= edge and
 *   vdw_scale * max_radius <= edge.  One wave per (complex, pose), one launch whatever n_pose; float64 arithmetic on the float32 inputs;
 *   an entry is the same bits alone, in any batch and among any n_pose. */
int fabind_protein_grid(const float* prot_xyz, const int* prot_z, const int* prot_off, int n_complex, const float* radii_in, float edge,
                        int* origin, int* dims, int* status, int* counts, const int* cell_off, const int* kept_off, int n_cells,
                        int n_kept, int* cell_of, int* cell_fill, int* slot, int* cell_ptr, float* xyz, float* radii, int* atom_id,
                        hipStream_t stream);
int fabind_pose_protein_check(const float* poses, int n_pose, int n_atoms, const int* atom_off, int n_complex, int max_atoms,
                              const int* plan_status, const float* lig_radii, const int* grid_status, const int* origin,
                              const int* dims, const int* cell_off, const int* kept_off, const int* cell_ptr, const float* xyz,
                              const float* radii, const int* atom_id, float edge, float cutoff, float clash_min, float overlap_max,
                              float vdw_scale, float spacing, float max_radius, float* stats, int* counts, int* pair, int* flags,
                              hipStream_t stream);
/* fabind_pose_relax (csrc/pose_relax.hip; a backward-compatible addition under ABI 19; fabind_amd/relax.py documents every layout): the
 * start conformer x0 fp32 [n_atoms, 3] of every ligand moved over its torsions (tor_off / quad / side of fabind_torsion_plan, t_total
 * rows; tor_off = NULL: rigid only) and one rigid motion, held to target fp32 [n_poses, n_atoms, 3] and pushed out of contact with the
 * kept protein atoms of the complex's cell list (fabind_protein_grid; grid_status = NULL or != 0: no protein term, status bit 16) and
 * out of its own PAIR_CLASH pairs (plan_status / cls uint32 [n_atoms, 16] / lig_radii of fabind_validity_plan; plan_status = NULL or
 * != 0: no intra term, status bit 8): damped Gauss-Newton on E = w_fit sum |X - y|^2 + w_prot sum max(0, c_prot (r_i + r_p) - d)^2 +
 * w_intra sum max(0, c_intra (r_i + r_j) - d)^2, started at angles0 fp32 [n_poses, t_total] (NULL: zeros) and the Horn fit onto the
 * target.  max_reach = c_prot * (largest ligand radius + largest protein radius) <= edge.  One wave per (complex, pose), one launch.
 * coords fp32 [n_poses, n_atoms, 3]; angles fp32 [n_poses, t_total] in (-pi, pi]; energy0 / energy fp64 [n_poses, n_complex, 3] = the
 * three unweighted sums at the start / the end; iters int32 [n_poses, n_complex] accepted steps; stop int32 [n_poses, n_complex] = 0
 * converged (E - E' <= tol E), 1 max_iters, 2 eight rejections in a row, 3 a non-finite input (NaN outputs); status int32 [n_complex] =
 * 0, 3 (more than 256 atoms: the Horn image, the last two sums NaN) or 4 (more than 58 torsions: relaxed rigidly, zero angles), plus
 * the bits 8 and 16; trace fp64 [n_poses, n_complex, max_iters] or NULL: E after each accepted step, NaN behind the last.  An entry is
 * the same bits alone, in any batch, among any n_poses and on a repeat. */
int fabind_pose_relax(const float* x0, const float* target, const float* angles0, const int* atom_off, int n_complex, int n_atoms,
                      int n_poses, const int* tor_off, const int* quad, const unsigned* side, int t_total, int max_atoms, int max_torsions,
                      const int* plan_status, const unsigned* cls, const float* lig_radii, const int* grid_status, const int* origin,
                      const int* dims, const int* cell_off, const int* kept_off, const int* cell_ptr, const float* prot_xyz,
                      const float* prot_radii, float edge, float max_reach, float w_fit, float w_prot, float w_intra, float c_prot,
                      float c_intra, int max_iters, float tol, float* coords, float* angles, double* energy0, double* energy, int* iters,
                      int* stop, int* status, double* trace, hipStream_t stream);
/* Start conformers from the bond list by distance geometry (csrc/embed.hip; fabind_amd/embed.py documents every layout and DESIGN.md
 * section 20 every rule).  Backward-compatible additions under ABI 19.
 * fabind_embed_bounds: per ligand (at most 256 heavy atoms) from the coded neighbour lists of fabind_torsion_plan and the atomic numbers z
 *   int32 [sum atoms]; chiral_sign int32 [sum atoms] (+1 / -1: the wanted sign of the stereo centre's signed volume, anything else:
 *   none) or NULL.  Count mode (quad_off = NULL): counts int32 [n_ligands] = signed-volume terms, status int32 [n_ligands] = 0 or 3 (more
 *   than 256 atoms: no entries).  Write mode (quad_off int32 [n_ligands + 1] = the exclusive sums of the counts, mat_off int64
 *   [n_ligands + 1] = the exclusive sums of n^2 over the ligands of status 0; status as the count pass left it): bounds fp32, one n x n
 *   block per ligand at mat_off (upper bound of (i, j) at (min, max), lower at (max, min), diagonal 0), triangle-smoothed in float32;
 *   geom int32 [sum atoms] = 0 TETRA / 1 TRIGONAL / 2 LINEAR; quads int32 [terms, 4] local ids with quad_lo / quad_hi fp32 [terms]: the
 *   interval of V = det[p1 - p0, p2 - p0, p3 - p0] (flat terms +-v_flat, stereo terms sign * [v_min, v_max]); status becomes 6 where
 *   some lower bound exceeds its upper bound after smoothing.  One work-group per ligand, no atomics.
 * fabind_embed_conformers: n_confs conformers of every ligand of status 0 under the bounds, one work-group per (ligand, conformer), every
 *   try and minimisation step inside the one launch.  keys uint32 [n_ligands]; coords fp32 [n_confs, n_atoms, 3] centred on the
 *   centroid; status int32 [n_ligands, n_confs] = 0, 1 (max_tries exhausted: the try of the smallest largest violation) or the plan's
 *   3 / 6 (zero rows); tries / steps int32, viol (largest pair violation, A) / energy fp64 [n_ligands, n_confs], all of the RETURNED
 *   coordinates; trace fp64 [n_ligands, n_confs, max_steps + 1] or NULL: E after each step of the last try, NaN behind the last.  An
 *   entry is the same bits alone, in any batch, among any n_confs and on a repeat. */
int fabind_embed_bounds(const int* nbr_ptr, const int* nbr_idx, const int* nbr_code, const int* atom_off, int n_ligands, const int* z,
                        const int* chiral_sign, float v_flat, float v_min, float v_max, int* counts, int* status, const int* quad_off,
                        const long long* mat_off, float* bounds, int* geom, int* quads, float* quad_lo, float* quad_hi,
                        hipStream_t stream);
int fabind_embed_conformers(const float* bounds, const long long* mat_off, const int* atom_off, int n_ligands, int n_atoms, int n_confs,
                            const int* plan_status, const int* quad_off, const int* quads, const float* quad_lo, const float* quad_hi,
                            const unsigned* keys, unsigned seed, int max_tries, int max_steps, int power_iters, float viol_tol,
                            float v_tol, float w_v, float w4, float* coords, int* status, int* tries, int* steps, double* viol,
                            double* energy, double* trace, hipStream_t stream);
/* Conformers of every ligand against each other or against reference conformers after the best rigid superposition
 * (csrc/conformer_rmsd.hip).  Backward-compatible additions under ABI 19.
 *   D = sqrt(min_k max(0, G_s + G_t - 2 lambda_k) / n_b): G the sums of squared distances to the own centroid, lambda_k the largest
 *   eigenvalue of Horn's 4 x 4 matrix of S_k = sum_i (x_s[a_k[i]] - c_s)(y_t[i] - c_t)^T, a_k the automorphisms of ligand b (atom_off,
 *   flat_off, auto_cnt, flat as fabind_pose_pair_rmsd takes them: auto_cnt[b] = 0 is the identity alone, an entry outside [0, n_b)
 *   counts as i).  Proper rotations only.  Centroids, centred coordinates, sums and the eigen-solve are double; D is fp32.
 * fabind_conformer_pair_rmsd: X fp32 [n_conf, n_atoms, 3] against itself -> D [n_ligands, n_conf, n_conf], every unordered pair computed
 *   once and mirrored, the diagonal +0.0.
 * fabind_conformer_cross_rmsd: X against Y fp32 [n_ref, n_atoms, 3] -> D [n_ligands, n_conf, n_ref] and, when auto_index / quat / trans
 *   are given (all three or none), per entry the minimising k (int32, the lowest on equal values), Horn's unit quaternion (w, x, y, z)
 *   fp64 [.., 4] and trans = c_t - R(q) c_s fp64 [.., 3]: R(q) x_s[a_k[i]] + trans is x_s superposed on y_t.
 * A ligand without atoms gets 0 (identity fit); one with more than max_atoms atoms gets NaN; a non-finite coordinate makes every entry of
 * its conformer NaN and no other.  An entry is the same bits alone, in any batch, among any n_conf / n_ref and on a repeat; no atomics.
 * n_conf, n_ref <= 512 and max_atoms (>= every n_b) <= 2048, refused otherwise before anything is launched. */
int fabind_conformer_pair_rmsd(const float* X, int n_conf, int n_atoms, const int* atom_off, const int* flat_off, const int* auto_cnt,
                               const int* flat, int n_ligands, int max_atoms, float* D, hipStream_t stream);
int fabind_conformer_cross_rmsd(const float* X, int n_conf, const float* Y, int n_ref, int n_atoms, const int* atom_off,
                                const int* flat_off, const int* auto_cnt, const int* flat, int n_ligands, int max_atoms, float* D,
                                int* auto_index, double* quat, double* trans, hipStream_t stream);
/* fabind_pose_score (csrc/pose_score.hip; a backward-compatible addition under ABI 19; fabind_amd/scoring.py documents every layout and
 * DESIGN.md section 22 every rule): the Vina-style intermolecular energy of poses fp32 [n_pose, n_atoms, 3] of the ligands atom_off int32
 * [n_complex + 1] against the kept atoms of the complex's cell list (fabind_protein_grid, built with edge >= cutoff), one launch, one
 * wave per (complex, pose).  lig_types int32 [n_atoms] and prot_types int32 [sum protein atoms] (read at prot_off[b] + atom_id) are
 * type words: radius class in bits 0-3 (C, N, O, P, S, F, Cl, Br, I, metal), 16 hydrophobic, 32 donor, 64 acceptor.  n_torsions int32
 * [n_complex] or NULL (0); params fp64 [6] on the device = the five weights and the torsion weight.  Pairs with r^2 < cutoff^2 in
 * float64; d = r - R_i - R_j.  terms fp32 [n_complex, n_pose, 5] = the unweighted sums (gauss1, gauss2, repulsion, hydrophobic, hbond),
 * inter = sum_k w_k term_k, total = inter / (1 + params[5] n_torsions) fp32 [n_complex, n_pose], n_pairs int32 [n_complex, n_pose],
 * per_atom fp32 [n_pose, n_atoms] or NULL: the weighted energy of every ligand atom, flags int32 [n_complex, n_pose]: 128 NONFINITE (a
 * NaN or infinite coordinate: every number of the pose NaN), 256 UNCHECKED (lig_status or grid_status != 0: NaN, no pairs).  Fixed
 * summation order, no atomics: an entry is the same bits alone, in any batch, among any n_pose and on a repeat. */
int fabind_pose_score(const float* poses, int n_pose, int n_atoms, const int* atom_off, int n_complex, int max_atoms,
                      const int* lig_status, const int* lig_types, const int* n_torsions, const int* grid_status, const int* origin,
                      const int* dims, const int* cell_off, const int* kept_off, const int* cell_ptr, const float* xyz,
                      const int* atom_id, const int* prot_off, const int* prot_types, float edge, float cutoff, const double* params,
                      float* terms, float* inter, float* total, int* n_pairs, float* per_atom, int* flags, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Cross attention (RowAttentionBlock / Attention._attention, models/cross_att.py:118-134,
 * models/model_utils.py:21-38,96-133).  Ragged: no padding, so the -1e9 mask bias never applies.
 *   for complex b, query i, key j, head h (4 heads x 32):
 *     s = scale * q[i,h,:].k[j,h,:] + lin*sigmoid(gate)   with (lin,gate) read from
 *         bias[(pair_off[b] + i*sq[b] + j*sk[b]) * bias_ld + {lin_col, gate_col} + h]
 *     out[i,h,:] = sigmoid(gpre[i,h,:]) * sum_j softmax_j(s) v[j,h,:]
 * desc: int32[B][8] = {q_off, nq, k_off, nk, pair_off_lo, pair_off_hi, sq, sk}.
 * ksplit > 1 splits the keys over work-groups (few queries, many keys: the ligand-query block); `part` =
 * float[n_rows * ksplit * 4 * 34] scratch, merged by a second kernel (out/lse rows are the first n_rows of q).
 * -------------------------------------------------------------------------------------------*/
int fabind_cross_attn_fwd(const float* q, int ldq, const float* k, const float* v, int ldkv, const float* gpre,
                          int ldg, const float* bias, int bias_ld, int lin_col, int gate_col, const int* desc, int B,
                          int max_nq, float scale, float* out, int ldo, float* lse, int ksplit, float* part, int n_rows,
                          hipStream_t stream);

/* Cross attention with the pair bias recomputed in the kernel (v1 stack; csrc/attn_mfma.hip, "fused" section): a work-group owns 64
 * protein rows of a complex, contracts their a0 rows (bf16 [rows, lda0], node-indexed) with the complex's packed ligand-side operand
 * `bo` (fabind_pair_bo_pack) on the matrix cores, forms bias = (lin + c) * sigmoid(gate + c') in registers and runs the attention of
 * fabind_cross_attn_mfma_fwd with it.  desc = int32[8] per complex {first protein row (node index), P, first ligand row (compact),
 * C, ...}; mode 0: queries = protein rows (q / gpre / out node-indexed, k / v compact ligand rows); mode 1: queries = ligand atoms
 * (q / gpre / out compact, k / v node-indexed), `part` = float[n_lig_rows * ceil(max_P / 64) * 4 * 34] scratch.  bconst = the eight
 * constants (lin0..3, gate0..3).  max_C <= 62.  Replaces RowAttentionBlock.forward incl. its pair-bias Linears (cross_att.py:118-134). */
/* lse (optional): receives the log-sum-exp of every (query row, head) -- what fabind_cross_attn_fused_bwd replays the weights from. */
int fabind_cross_attn_fused_fwd(const float* q, int ldq, const float* k, const float* v, int ldkv, const float* gpre, int ldg,
                                const void* a0, int lda0, const void* bo, const int* toff, const float* bconst, const int* desc, int B,
                                int max_P, int max_C, int H, int mode, float scale, float* out, int ldo, float* part, int n_lig_rows,
                                float* lse, hipStream_t stream);
/* bo[(toff[b] * H/32 + ks * T_b + tile) * 512 + lane * 8 + e] = b0[c_index[lig0_b + atom], k] * wcomp[slot_row, k] in MFMA fragment
 * order (tile = 16 columns = 2 atoms x {lin0, gate0, lin1, gate1, lin2, gate2, lin3, gate3}; T_b = ceil(C_b / 2); toff = prefix sum of
 * T_b; tile_b[t] = complex of global tile t); wcomp = fp32 [8, H] rows lin0..3, gate0..3 (the composed weights W_{lin|gate} W_o). */
int fabind_pair_bo_pack(const float* b0, int ldb, const float* wcomp, int H, const int* c_index, const int* desc, const int* toff,
                        const int* tile_b, int n_tiles, void* out, int n_blocks, long blk_stride, hipStream_t stream);
/* (n_blocks packs in one launch: block k reads wcomp + k * 8 * H and writes out + k * blk_stride elements) */

/* Fused BACKWARD of the same block (round 4): the bias is recomputed on the matrix cores in both passes, the per-pair gradients
 * D = (d lin_h, d gate_h)_h never leave the chip as fp32 -- they overwrite the LDS bias tile as bf16, are contracted with the packed
 * operand `boT` (fabind_pair_bot_pack) for  d a0 += D Bo  in the kernel, and go out as bf16 rows of `acat` (row = compact protein
 * index, columns kcol0 + atom * 8 + slot, slot order lin0, gate0, lin1, gate1, ...) for the T = D^T a0 contraction that the ligand-side
 * and weight gradients need over ALL row tiles of a complex (fabind_batched_transpose_pad + fabind_gemm + fabind_pair_bias_finish,
 * as on the tensor path).  Replaces autograd of cross_att.py:118-134 / model_utils.py:21-38,96-159 for the v1 stack.
 * qg = q | gate pre-activations of the QUERY side [rows, ldq >= 256] (mode 0: protein rows in the node layout; mode 1: compact ligand
 * rows), kv = k | v of the KEY side, out / dout = the forward's output and its gradient [query rows, 128], lse = the forward's
 * log-sum-exp [query rows, 4]; outputs: dqg [query rows, ldq] (d q | d gate-pre), dkv [key rows, ldkv], scratch dO [query rows, 128],
 * Dv [query rows, 4]; da0 (optional: +=, fp32 [N, ldda0], columns [0, H); NULL: the caller contracts `acat` with fabind_pair_bias_btcat's operand), colpart = fabind_cross_attn_fused_bwd_parts(B, max_P) rows of ldcolpart >= 8
 * floats (per-tile column sums of D in the first 8 of a row: their sum is d bconst in slot order), part = float[fabind_cross_attn_fused_bwd_scratch(...)].
 * desc = the forward's descriptors, desc_p = int32[8] per complex whose first entry is the complex's first row in the compact protein
 * list; toff / koff = int32[B + 1] prefix sums of ceil(C / 2) / ceil(C / 4).  nsplit, B, part_rows are filled in by the library. */
typedef struct FabindAttnFusedBwdArgs {
    const float* qg; const float* kv; const void* a0; const void* bo; const void* boT; const int* toff; const int* koff;
    const float* bconst; const int* desc; const int* desc_p; const float* out; const float* lse; const float* dout;
    float* dqg; float* dkv; float* dO; float* Dv; float* da0; void* acat; float* colpart; float* part;
    int ldq, ldkv, lda0, ldda0, ldacat, kcol0, ldcolpart, kp;   /* kp: width of this block's column range of acat (>= max_C * 8; the tail is zero-filled) */
    float scale;
    int nsplit, B, part_rows;
} FabindAttnFusedBwdArgs;
int fabind_cross_attn_fused_bwd(const FabindAttnFusedBwdArgs* args, int B, int max_P, int max_C, int H, int mode, int n_lig_rows,
                                hipStream_t stream);
long fabind_cross_attn_fused_bwd_scratch(int B, int max_P, int max_C, int n_lig_rows, int mode);
int fabind_cross_attn_fused_bwd_parts(int B, int max_P);
/* boT[((koff[b] + ks) * (H / 16) + nt) * 512 + lane * 8 + e] = b0[atom][h] * wcomp[(e & 1) * 4 + (e >> 1)][h], atom = ks * 4 + (lane >> 4),
 * h = nt * 16 + (lane & 15) (zero rows past C): the A operand of the kernel's d a0 contraction.  kstep_b = int32[n_ksteps]: complex of
 * every k-step. */
int fabind_pair_bot_pack(const float* b0, int ldb, const float* wcomp, int H, const int* c_index, const int* desc, const int* koff,
                         const int* kstep_b, int n_ksteps, void* out, int n_blocks, long blk_stride, hipStream_t stream);

/* The same block with QK^T and softmax.V on the matrix cores (v_mfma_f32_16x16x32_bf16: head dim 32 = one instruction per
 * 16-key x 16-query tile; csrc/attn_mfma.hip): identical arguments, results and partials layout; q / k / v / probabilities
 * are rounded to bf16 as MFMA operands, scores, pair bias, softmax statistics and outputs stay fp32.  bias_ld, lin_col and
 * gate_col must be multiples of 4 (a pair's four heads are read as one 16-byte segment). */
int fabind_cross_attn_mfma_fwd(const float* q, int ldq, const float* k, const float* v, int ldkv, const float* gpre, int ldg,
                               const float* bias, int bias_ld, int lin_col, int gate_col, const int* desc, int B, int max_nq,
                               float scale, float* out, int ldo, float* lse, int ksplit, float* part, int n_rows,
                               hipStream_t stream);

/* pair-bias precompute helpers (RowAttentionBlock.linear/linear_g applied to the initial pair
 * embedding z0 = W_o (a_i * b_j) + b_o; models/cross_att.py:125, models/att_model.py:198-206):
 * bmat[(j*NO + o), k] = b0[c_node(j), k] * wcomp[o, k]  for the ligand-side rows of one batch. */
int fabind_pair_bmat(const float* b0, int ldb, const float* wcomp, int NO, int H, const int* c_node, int n_c,
                     void* bmat, int bmat_dt, hipStream_t stream);
/* hd[e, 0:H] = a0[red_p[e]]*b0[red_c[e]],  hd[e, H:H+H2] = a1[red_p[e]]*b1[red_c[e]]  */
int fabind_pair_hadamard(const float* a0, const float* b0, int ld0, int H, const float* a1, const float* b1, int ld1,
                         int H2, const int* red_p, const int* red_c, int n_red, void* hd, int hd_dt, int ldh,
                         hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Inter-graph attention layer (MC_Att_L.att_model/node_model/coord_model, models/egnn.py:186-252)
 * on node-level projections qkv[N,3H] = [q | k | v] and cv[N,H] = coord_mlp.0(v) :
 *   logit_e = q[r].(k[c] + rhohat_e w_rk) + sum_k bias_red[red_idx[e], k]   (row-dot partials; any
 *             per-layer constant offset cancels in the softmax and is dropped)
 *   alpha   = segment softmax over the row
 *   h_out[r] = h[r] + sum_e alpha_e (v[c] + rhohat_e w_rv)
 *   x_out[r] = x[r] + clamp( sum_e d_e alpha_e * w3.silu(cv[c] + rhohat_e wcr), +-clampv )
 * -------------------------------------------------------------------------------------------*/
int fabind_inter_attn_fwd(const float* qkv, int ldqkv, const float* cv, int ldcv, int H, const float* h, int ldh,
                          const float* x, const float* d, const float* rhohat, const int* rowptr, const int* col,
                          const int* red_idx, const float* bias_red, int bias_np, const float* w_rk,
                          const float* w_rv, const float* wcr, const float* w3, float clampv, int n_rows,
                          float* h_out, float* x_out, float* alpha, float* cvs,
                          const float* s_ext /* optional per-edge scalar added to the coord_mlp value (FABind+: its coord_mlp is an
                                                LN-MLP evaluated outside); its gradient is the backward's dcp[] */,
                          void* h16 /* NULL, or [n_rows, H] bf16: h_out as the next contraction's operand */,
                          hipStream_t stream);
/* The same with the rows DEALT BY DEGREE (round 5, csrc/inter_attn_rows.hip): `order` [n_rows] int32 = the rows sorted by their number of
 * inter edges, descending (stable); order[0 .. n_heavy) are the rows with more than 8 edges -- one work-group of four waves each, a
 * contiguous quarter of the row's edges per wave, log-sum-exp combine in wave order --, order[n_heavy .. n_act) the other rows with edges
 * (one wave each), order[n_act .. n_rows) the rows without edges (pass-through).  Same results up to the summation order of a heavy row;
 * deterministic.  fabind_inter_attn_bwd_rows is the adjoint on the same deal. */
int fabind_inter_attn_fwd_rows(const float* qkv, int ldqkv, const float* cv, int ldcv, int H, const float* h, int ldh,
                               const float* x, const float* d, const float* rhohat, const int* rowptr, const int* col,
                               const int* red_idx, const float* bias_red, int bias_np, const float* w_rk,
                               const float* w_rv, const float* wcr, const float* w3, float clampv, int n_rows,
                               float* h_out, float* x_out, float* alpha, float* cvs, const float* s_ext, void* h16,
                               const int* order, int n_heavy, int n_act, hipStream_t stream);

/* LAS geometry step (models/egnn.py:433-449): x_out = x + clamp(step * sum_{(i,j): j=node} 4(|xi-xj|^2-|x0i-x0j|^2)(xi-xj)).
 * las_off[B+1]: per-complex ranges of the (complex-contiguous) LAS edge list.
 * pass_mask [N] (optional, NULL in forward-only passes): per moved atom, bit k set = component k of the update was inside the clamp
 * (what fabind_las_step_bwd reads; every node's entry is written, 0 for the nodes that are not ligand atoms). */
int fabind_las_step(const float* x, const float* x0, const int* las_i, const int* las_j, const int* las_off,
                    const int* node_off, const int* c_cnt, int B, int max_n, float step, float clampv, float* x_out,
                    unsigned char* pass_mask, hipStream_t stream);

/* Pocket centre (models/model.py:146-158): per complex b over its L (padded) residues
 *   s = sigmoid(logit); p = clamp([1 - s, s], 1e-6, 1 - 1e-6); y = softmax((log p + noise) / tau) over the two classes
 *   (noise: the Gumbel samples of F.gumbel_softmax in train mode, [B, L, 2], NULL in eval = utils/utils.py:687-699 gumbel_softmax_no_random);
 *   hard != 0: the straight-through one-hot; w = y[..., 1] * mask; center[b] = sum_l w_l xyz[b, l] / sum_l w_l; wsum[b] = sum_l w_l.
 * logits / mask: [B, L] (fp32 / uint8), xyz [B, L, 3].  _bwd: dlogits [B, L] from dcenter [B, 3] (the soft path's gradient; 0 at masked
 * positions).  One launch each; fixed-order sums. */
int fabind_pocket_center_fwd(const float* logits, const uint8_t* mask, const float* xyz, const float* noise, int B, int L,
                             float tau, int hard, float* center, float* wsum, hipStream_t stream);
int fabind_pocket_center_bwd(const float* logits, const uint8_t* mask, const float* xyz, const float* noise, int B, int L,
                             float tau, const float* center, const float* wsum, const float* dcenter, float* dlogits,
                             hipStream_t stream);

/* Training loss (main_fabind.py:398-417), all six terms and their sum in ONE launch:
 *   out[0] pocket_cls      = w_cls * BCEWithLogits(logits, cls) (mean over all n_cls = B * Lmax positions, padding included) * n_cls / sum(mask)
 *   out[1] pocket_center   = w_center * Huber_delta(center, center_true)                (mean over n_center = 3 B)
 *   out[2] contact         = w_pair * MSE(y_pred, dis_map)      out[3] contact_by_pred = w_pair * MSE(y_by, dis_map)
 *   out[4] distill         = w_distill * MSE(y_by, y_pred)      out[5] coord = w_coord * SmoothL1(coords, coords_true)   (n_coord = 3 * atoms)
 *   out[6] = their sum (in this order), out[7] = sum(mask); loss_out[1] / terms_out[6] (either may be NULL): copies of out[6] / out[0..5].
 * cls_dt: dtype of `cls`: 0 fp32, 1 int64, 2 int32, 3 uint8.  part: fp32 scratch [fabind_loss_blocks(n_pair, n_coord, n_cls)][8];
 * ticket: one uint32 that is ZERO before the first launch (the kernel re-arms it).  Deterministic (block partials summed in block order).
 * fabind_loss_bwd: the gradient seeds d_coords / d_y_pred / d_y_by / d_logits / d_center (any may be NULL) for the upstream gradients
 * g_loss (scalar, of out[6]) and g_terms[6] (of out[0..5]); either may be NULL (= 0).  fwd_out = the forward's out[8]. */
int fabind_loss_blocks(long n_pair, long n_coord, long n_cls);
int fabind_loss_fwd(const float* coords, const float* coords_true, long n_coord, const float* y_pred, const float* y_by,
                    const float* dis_map, long n_pair, const float* logits, const void* cls, int cls_dt, const uint8_t* mask,
                    long n_cls, const float* center, const float* center_true, long n_center, float w_coord, float w_pair,
                    float w_distill, float w_cls, float w_center, float delta, float* part, unsigned* ticket, float* out,
                    float* loss_out, float* terms_out, hipStream_t stream);
int fabind_loss_bwd(const float* coords, const float* coords_true, long n_coord, const float* y_pred, const float* y_by,
                    const float* dis_map, long n_pair, const float* logits, const void* cls, int cls_dt, long n_cls,
                    const float* center, const float* center_true, long n_center, float w_coord, float w_pair, float w_distill,
                    float w_cls, float w_center, float delta, const float* fwd_out, const float* g_loss, const float* g_terms,
                    float* d_coords, float* d_y_pred, float* d_y_by, float* d_logits, float* d_center, hipStream_t stream);

/* Pair operations of the distance-map head (models/model.py:344-365; SURVEY K19 glue) on per-complex BLOCK descriptors: the valid
 * (pocket residue i, ligand atom j) pairs of complex b are the dense block P_b x C_b, protein-major, at pair index pair_off + i * C_b + j
 * (z[z_mask] of the reference's padded [B, P, C] tensors).  desc: device array of B records
 *   struct { int64 pair_off; int32 P, C, p_row0, c_row0, tile0, pad; }      (32 bytes; tile0 = first of the complex's ceil(P / TP) tiles,
 *   TP = fabind_pair_block_tile()), n_tiles = sum_b ceil(P_b / TP).
 * fabind_pair_dist_fwd: y[pair] = clamp(scale * |xp[p_row0 + i] - xc[c_row0 + j]|, lo, hi)   (torch.cdist -> [z_mask] -> unnormalize -> clamp,
 *   model.py:349,363-365).  _bwd: dxc[c_row0 + j] (rows of every complex's atoms; fixed-order sums); part: fp32 scratch [B][8][max_C][3].
 * fabind_block_hadamard_bwd: adjoint of out[pair, :] = tp[p_row0 + i, :] * tc[c_row0 + j, :] (einsum 'bik,bjk->bijk' on the valid pairs,
 *   model.py:355) for a bf16 dout [pairs, W] (W in {64, 128, 256, 512}): dtp / dtc rows written once each, no atomics;
 *   row_b[n_crows]: complex of every row of tc; nchunk_max = ceil(max_b C_b / fabind_pair_block_chunk());
 *   part: fp32 scratch [n_tiles][nchunk_max][chunk][W]. */
int fabind_pair_block_tile(void);
int fabind_pair_block_chunk(void);
int fabind_pair_dist_fwd(const void* desc, int B, int n_tiles, const float* xp, const float* xc, float scale, float lo, float hi,
                         float* y, hipStream_t stream);
int fabind_pair_dist_bwd(const void* desc, int B, int max_C, const float* xp, const float* xc, const float* dy, float scale, float lo,
                         float hi, float* part, float* dxc, hipStream_t stream);
int fabind_block_hadamard_fwd(const void* desc, int B, int n_tiles, const float* tp, int ldtp, const float* tc, int ldtc, int W, void* out,
                              int ldo, hipStream_t stream);      /* out[pair, :] = bf16(tp[p_row0 + i, :] * tc[c_row0 + j, :]) */
int fabind_block_hadamard_bwd(const void* desc, int B, int n_tiles, const void* dout, int ldo, const float* tp, int ldtp,
                              const float* tc, int ldtc, int W, const int* row_b, int n_crows, int nchunk_max, float* part,
                              float* dtp, int lddp, float* dtc, int lddc, hipStream_t stream);

/* x_out[i] = mask[i] ? z[i] : x[i]   (X[mask] = Z[mask], models/att_model.py:236,245) */
int fabind_select_rows(const float* x, const float* z, const uint8_t* mask, int n, int width, float* x_out,
                       hipStream_t stream);

/* LayerNorm over the last dim (models/model.py:15,29): y = (x-mean)*rstd*w + b; backward returns dx and
 * per-block partial sums of dw/db ([ceil(R/4), C] each, reduce with fabind_colsum). */
/* Per-row LayerNorm statistics without writing the normalised rows: mu[r] = mean, rs[r] = rsqrt(centred variance + eps)
 * of x[r, 0:C] (two passes over registers, like fabind_layernorm_rows).  Feeds the row_mu / row_rs fold of fabind_gemm. */
int fabind_row_stats(const void* x, int x_dt, int ldx, float eps, int R, int C, float* mu, float* rs, hipStream_t stream);

/* FABind+ LN-MLPs (FABind_plus/fabind/models/model_utils.py:10-74).  fabind_layernorm_rows: row LayerNorm with free
 * input / output dtypes (FB_DT_*) and strides; output columns [C, pad_to) are zero-filled (GEMM K padding).
 * fabind_edge_ln_concat: LayerNorm over the concatenated edge input [h[row] | h[col] | rhohat] (2H+1 columns,
 * FABind_plus/fabind/models/egnn.py:52-58) evaluated while gathering. */
int fabind_layernorm_rows(const void* x, int x_dt, int ldx, const float* w, const float* b, float eps, int R, int C, void* y,
                          int y_dt, int ldy, int pad_to, hipStream_t stream);
int fabind_edge_ln_concat(const float* h, int ldh, int H, const int* row, const int* col, const float* rhohat, const float* w,
                          const float* b, float eps, int E, void* y, int y_dt, int ldy, int pad_to, hipStream_t stream);

/* First Linear of FABind+'s LN-MLP edge model (egnn.py:52-58, model_utils.py:44-46) with the LayerNorm folded into
 * per-node projections, bf16 inference:
 *   out[e,:] = drop(relu( rs_e * (AB[row[e], 0:Kp] + AB[col[e], Kp:2Kp] + (m_r-mu_e) c_r + (m_c-mu_e) c_c + (rho[e]-mu_e) w_r) + dvec ))
 * AB = bf16 [nodes, ldab] = (h - m 1^T) [W1 diag(ln_w)]_{r|c}^T (node-centred features), stat = fp32 [nodes][2] =
 * (mean m, centred sum of squares) of each node's H features; (mu_e, rs_e) are the LayerNorm statistics of
 * [h_r | h_c | rho] (2H+1 values) combined from them; c_r / c_c = row sums of the two weight blocks.  out = bf16 [E, Kp].
 * Dropout mask: hash32(seed + e*Kp + c) & 0xffff >= round(p*65536). */
int fabind_edge_lnfold(const void* AB, int ldab, int Kp, int H, const int* row, const int* col, const float* rho,
                       const float* stat, float eps, const float* w_r, const float* c_r, const float* c_c, const float* dvec,
                       int E, void* out, float p_drop, unsigned seed, hipStream_t stream);
/* Adjoint of fabind_edge_lnfold (round 5: the folded first edge Linear under autograd): out = what the forward wrote (its zeros are the
 * inactive and the dropped positions), dout = its gradient (bf16 [E, Kp]).  Writes du = rs_e x dout x mask x 1/(1-p) as bf16 [E, Kp] (the
 * caller's segment sums over the receiving / sending node give the gradient of AB's two halves), es = fp32 [E][8] = (d m_r, d Q_r, d m_c,
 * d Q_c, 0, 0, 0, 0): the gradients of the receiving / sending node's statistics through this edge, drho [E], and part = fp32 [n_blocks][4][Kp]
 * partial column sums (d dvec, d c_r, d c_c, d w_r); n_blocks = fabind_edge_lnfold_bwd_blocks(E).  Kp <= 1536. */
int fabind_edge_lnfold_bwd_blocks(int E);
int fabind_edge_lnfold_bwd(const void* AB, int ldab, int Kp, int H, const int* row, const int* col, const float* rho,
                           const float* stat, float eps, const float* w_r, const float* c_r, const float* c_c,
                           const void* out, const void* dout, int E, float p_drop, void* du, float* es,
                           float* drho, float* part, int n_blocks, hipStream_t stream);

/* coord_mlp of FABind+'s inter-edge attention layer (egnn.py:277-300; LN -> Linear -> relu -> dropout -> bias-free Linear)
 * on the value rows v_e = V[col] + rho * w_rv, LayerNorm folded into a per-node projection, bf16 inference:
 *   s_out[e] = sum_k w3[k] * drop(relu( rs_e * (P[col[e], k] + rho[e] * u[k]) + d[k] )),
 *   rs_e = rsqrt( (stat[col][0] + 2 rho stat[col][1] + rho^2 q_w) / H + eps )
 * P = bf16 [nodes, ldp] = (V - mean 1^T)(W1 diag(ln_w))^T; stat = fp32 [nodes][2] = (|Vc|^2, Vc . wc); wc = w_rv - mean(w_rv),
 * q_w = |wc|^2, u = W1 diag(ln_w) wc, d = W1 ln_b + b1.  H % 8 == 0, H <= 512.
 * Dropout mask: hash32(seed + e*H + k) & 0xffff >= round(p*65536). */
int fabind_inter_coord_fold(const void* P, int ldp, int H, const int* col, const float* rho, const float* stat, float q_w,
                            float eps, const float* u, const float* d, const float* w3, int E, float* s_out, float p_drop,
                            unsigned seed, hipStream_t stream);
/* adjoint of fabind_layernorm_rows: dx (dtype dx_dt, leading dim lddx) and per-work-group partials of dw, db ([nblk][C] each;
 * nblk = the grid the caller chooses, one wave per row strided over it -- every partial row is written; the caller adds the rows).  fabind_edge_concat: y[e] = [h[row[e]] | h[col[e]] | rhohat[e] | 0...]
 * (the un-normalised edge input of MC_E_GCL, used under autograd where LayerNorm is a separate differentiable step). */
int fabind_layernorm_rows_bwd(const void* x, int x_dt, int ldx, const float* w, const void* dy, int dy_dt, int lddy, float eps,
                              int R, int C, void* dx, int dx_dt, int lddx, float* dw_part, float* db_part, int nblk, hipStream_t stream);
int fabind_edge_concat(const float* h, int ldh, int H, const int* row, const int* col, const float* rhohat, int E, void* y,
                       int y_dt, int ldy, int pad_to, hipStream_t stream);
int fabind_layernorm_fwd(const float* x, const float* w, const float* b, float eps, int R, int C, float* y, float* mean,
                         float* rstd, hipStream_t stream);
int fabind_layernorm_bwd(const float* x, const float* w, const float* dy, const float* mean, const float* rstd, int R,
                         int C, float* dx, float* dw_part, float* db_part, hipStream_t stream);

/* Form report of the normalisation launchers: which kernel and template instantiation a call would run, answered by the same host
 * function the launcher itself dispatches through, without launching anything (host code only: pointers are looked at for their
 * alignment and never dereferenced).  Every argument is the launcher's argument of that name.  The *_COUNT values close each list. */
/* fabind_layernorm_rows.  Rows per work-group: 16 (8S16), 8 (8S32), 4 elsewhere. */
#define FB_LNR_8S16 0  /* layernorm_rows8s_kernel<16>: 8-column accesses, C <= 128, four rows per wave */
#define FB_LNR_8S32 1  /* layernorm_rows8s_kernel<32>: 8-column accesses, 128 < C <= 256, two rows per wave */
#define FB_LNR_V8_1 2  /* layernorm_rows8_kernel<1>:   8-column accesses, 256 < C <= 512 */
#define FB_LNR_V8_2 3  /* layernorm_rows8_kernel<2>:   512 < C <= 1024 */
#define FB_LNR_V8_3 4  /* layernorm_rows8_kernel<3>:   1024 < C <= 1536 */
#define FB_LNR_V8_4 5  /* layernorm_rows8_kernel<4>:   1536 < C <= 2048 */
#define FB_LNR_S2 6    /* layernorm_rows_kernel<2>:    scalar accesses (a leading dimension, pad_to or an address rules out 8 columns), C <= 128 */
#define FB_LNR_S8 7    /* layernorm_rows_kernel<8>:    128 < C <= 512 */
#define FB_LNR_S16 8   /* layernorm_rows_kernel<16>:   512 < C <= 1024 */
#define FB_LNR_S32 9   /* layernorm_rows_kernel<32>:   1024 < C <= 2048 */
#define FB_LNR_COUNT 10
int fabind_layernorm_rows_form(const void* x, int ldx, int C, const void* y, int ldy, int pad_to);
/* fabind_layernorm_rows_bwd.  Every form strides rows over the caller's nblk work-groups of four waves (8S16: 16 rows per work-group and
 * trip, 8S32: 8, elsewhere 4). */
#define FB_LNB_8S16 0  /* layernorm_rows_bwd8s_kernel<16>: 8-column accesses, C <= 128 */
#define FB_LNB_8S32 1  /* layernorm_rows_bwd8s_kernel<32>: 128 < C <= 256 */
#define FB_LNB_V8_1 2  /* layernorm_rows_bwd8_kernel<1>:   256 < C <= 512 */
#define FB_LNB_V8_2 3  /* layernorm_rows_bwd8_kernel<2>:   512 < C <= 1024 */
#define FB_LNB_V8_3 4  /* layernorm_rows_bwd8_kernel<3>:   1024 < C <= 1536 */
#define FB_LNB_S2 5    /* layernorm_rows_bwd_kernel<2>:    scalar accesses, C <= 128 */
#define FB_LNB_S8 6    /* layernorm_rows_bwd_kernel<8>:    128 < C <= 512 */
#define FB_LNB_S16 7   /* layernorm_rows_bwd_kernel<16>:   512 < C <= 1024 */
#define FB_LNB_S20 8   /* layernorm_rows_bwd_kernel<20>:   1024 < C <= 1280 */
#define FB_LNB_S32 9   /* layernorm_rows_bwd_kernel<32>:   1280 < C <= 2048 (also every 8-column-capable shape beyond C = 1536) */
#define FB_LNB_COUNT 10
int fabind_layernorm_rows_bwd_form(const void* x, int ldx, const void* dy, int lddy, const void* dx, int lddx, int C);
/* fabind_row_stats */
#define FB_RST_BF16_1 0   /* row_stats_bf16_kernel<1>: bf16 rows, C % 8 == 0, 16-byte aligned, C <= 512 */
#define FB_RST_BF16_2 1   /* row_stats_bf16_kernel<2>: 512 < C <= 1024 */
#define FB_RST_BF16_4 2   /* row_stats_bf16_kernel<4>: 1024 < C <= 2048 */
#define FB_RST_GENERIC 3  /* row_stats_kernel: every other dtype / shape, two element-wise passes */
#define FB_RST_COUNT 4
int fabind_row_stats_form(const void* x, int x_dt, int ldx, int C);
/* fabind_edge_lnfold.  *edges_per_trip (may be NULL) receives U, the edges a wave takes per trip of its walk over the
 * 4 x fabind_edge_lnfold_blocks(E) waves of the grid (0 for the per-chunk kernel, which does not walk). */
#define FB_ELF_WAVE1 0       /* edge_lnfold_wave_kernel<1, ELF_U1, false>: H % 4 == 0, Kp / 8 <= 64: every chunk of the row in one pass */
#define FB_ELF_WAVE1_TAIL 1  /* edge_lnfold_wave_kernel<1, ELF_U1, true>:  H <= 256, Kp / 8 > 64: 2H leading columns + a tail pass */
#define FB_ELF_WAVE2_TAIL 2  /* edge_lnfold_wave_kernel<2, ELF_U2, true>:  256 < H <= 512 */
#define FB_ELF_CHUNK 3       /* edge_lnfold_kernel: one thread per (edge, 8-column chunk): H % 4 != 0, H > 512 or a tail beyond 64 chunks */
#define FB_ELF_COUNT 4
int fabind_edge_lnfold_form(int Kp, int H, int* edges_per_trip);
int fabind_edge_lnfold_blocks(int E);
/* fabind_edge_lnfold_bwd (grid: fabind_edge_lnfold_bwd_blocks(E) work-groups of four waves) */
#define FB_ELB_NPL1 0  /* edge_lnfold_bwd_kernel<1, ELB_U1>: Kp <= 512 */
#define FB_ELB_NPL2 1  /* edge_lnfold_bwd_kernel<2, ELB_U2>: 512 < Kp <= 1024 */
#define FB_ELB_NPL3 2  /* edge_lnfold_bwd_kernel<3, ELB_U3>: 1024 < Kp <= 1536 */
#define FB_ELB_COUNT 3
int fabind_edge_lnfold_bwd_form(int Kp, int* edges_per_trip);
/* grid of fabind_inter_coord_fold: four waves per work-group, one edge per wave and trip */
int fabind_inter_coord_fold_blocks(int E);

/* elementwise: out = a + b (fp32), n elements */
int fabind_add(const float* a, const float* b, float* out, long n, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Backward passes (adjoints of the kernels above; they replace torch autograd's traversal of the
 * reference's ATen/torch_scatter graph for the same ops).  Contractions in backward passes go through
 * fabind_gemm / fabind_transpose_act / fabind_colsum.
 * -------------------------------------------------------------------------------------------*/
int fabind_mul_dact(const void* dy, int dy_dt, const void* y, int y_dt, int act, void* out, int out_dt, long n, float scale,
                    hipStream_t stream);
/* out = scale * dy * act'(y) (y = NULL with FB_ACT_NONE: dtype conversion) and colsum[c] = sum_r out[r,c] in one pass
 * (bias gradient of the Linear whose activation is being undone); [R,C] contiguous, scratch [nchunk, C].
 * scale: 1, or keep^-1 = 1 / (1 - p) when y is the output of a ReLU epilogue WITH dropout (fabind_gemm p_drop): y = relu(pre) keep / (1 - p),
 * so d y / d pre = [y > 0] / (1 - p) -- the dropped positions are exactly the zeros of y, no mask is stored or recomputed. */
int fabind_mul_dact_colsum(const void* dy, int dy_dt, const void* y, int y_dt, int act, void* out, int out_dt, int R, int C,
                           float* colsum, float* scratch, int nchunk, float scale, hipStream_t stream);
/* out [R,C] = dy * keep(seed, r, c) / (1 - p) and its column sums: the adjoint of fabind_gemm's epilogue dropout (key seed + r * C + c,
 * C = the GEMM's N) where the saved output does not show the mask -- dropout AHEAD of a residual (the train-mode sites of the
 * reference: nn.Dropout on the node-MLP output / the attention update before `h + ...`, FABind/fabind/models/egnn.py:106,
 * cross_att.py:128) or without an activation.  Nothing is stored by the forward: the mask is regenerated from its key. */
int fabind_mul_dropmask_colsum(const void* dy, int dy_dt, void* out, int out_dt, int R, int C, float p_drop, unsigned seed,
                               float* colsum, float* scratch, int nchunk, hipStream_t stream);
/* out = h + drop(hn - h) over n fp32 elements (nn.Dropout on the aggregated inter-edge attention message ahead of the residual,
 * FABind/fabind/models/egnn.py:236) and its adjoint (d hn = g keep / (1 - p), d h = g - d hn): the counter-based mask of the GEMM
 * epilogues keyed by (seed, linear index), regenerated by the adjoint. */
int fabind_drop_mix(const float* h, const float* hn, float* out, long n, float p_drop, unsigned seed, hipStream_t stream);
int fabind_drop_mix_bwd(const float* g, float* dhn, float* dh, long n, float p_drop, unsigned seed, hipStream_t stream);
int fabind_rowdot_bwd(const void* z, int z_dt, const float* dpart, int np, const float* u, int act, int M, int N,
                      void* dz, float* du, float* scratch, int nchunk, hipStream_t stream);
int fabind_edge_geom_bwd(const float* d, const float* rho, const float* norm, const float* dd, const float* drhohat,
                         const int* row, const int* rowptr, const int* colptr /* edges grouped by sending node */,
                         const int* perm /* their edge ids */, const int* node_off, int B, int E, int n_nodes, float* dx,
                         float* g_scratch /* [E,3] */, float* T_scratch /* [B] */, hipStream_t stream);
int fabind_gcl_pre_bwd(const void* dpre, int dt, int H, const float* rhohat, const float* w_r, int E, float* drh,
                       float* dw, float* scratch, int nchunk, hipStream_t stream);
int fabind_gather_dact(const float* dout, int ldo, const int* row, const void* Z, int z_dt, int act, void* dZ, int dz_dt,
                       int E, int H, hipStream_t stream);
int fabind_coord_update_bwd(const float* d, const float* s, const int* rowptr, int n_rows, int mean, float clampv,
                            const float* dxo, float* dd, float* ds, hipStream_t stream);
/* Adjoint of fabind_cross_attn_fwd.  Writes dqg / dkv / dbias only at the rows / pairs the block descriptors cover (the caller
 * zero-initialises them if other rows exist).  When one side has <= 256 rows per complex and the other >= 512, the long loop of
 * the short side is split over work-groups; the per-split partial sums go through `scratch` (fabind_cross_attn_bwd_scratch()
 * floats, fp32) and are added by a reduce kernel -- no float atomics, the result is deterministic. */
long fabind_cross_attn_bwd_scratch(int B, int max_nq, int max_nk);
int fabind_cross_attn_bwd(const float* qg, int ldq, const float* kv, int ldkv, const float* bias, int bias_ld,
                          int lin_col, int gate_col, const int* desc, int B, int max_nq, int max_nk, float scale,
                          const float* out, const float* lse, const float* dout, float* dqg, float* dkv, float* dbias,
                          float* dO, float* Dv, float* scratch, hipStream_t stream);
/* MFMA bf16 form of the same adjoint (csrc/attn_mfma.hip): same arguments and scratch size; dO, dS and the recomputed
 * probabilities enter the contractions as bf16, dbias / dq / dk / dv are accumulated and written in fp32. */
int fabind_cross_attn_mfma_bwd(const float* qg, int ldq, const float* kv, int ldkv, const float* bias, int bias_ld,
                               int lin_col, int gate_col, const int* desc, int B, int max_nq, int max_nk, float scale,
                               const float* out, const float* lse, const float* dout, float* dqg, float* dkv, float* dbias,
                               float* dO, float* Dv, float* scratch, hipStream_t stream);
/* Operands of the pair-bias adjoint (autograd of the pair bias of RowAttentionBlock, cross_att.py:125, all attention blocks at
 * once) concatenated along K, bf16:  Acat[poff_b + i, k*Kp + j*8 + o] = douts[k][pair(b,i,j), o],
 * BTcat[b*H + h, k*Kp + j*8 + o] = b0[ligand j of b, h] * wcomp[k][o][h]  (zeros for j >= C_b; Kp = 8 * max_C rounded up to 32).
 * douts: HOST array of nblk device pointers (fp32 [n_pairs, 8] each, NULL = no gradient); desc_p: the block descriptors of
 * fabind_cross_attn_fwd with the protein side compact; lda must be nblk*Kp (Acat rows are written contiguously).  colpart
 * (optional): fp32 [fabind_pair_bias_cat_parts(B, max_P)][nblk*8], one row of partial column sums of the douts per work-group --
 * their sum over the rows is the gradient of the pair-bias constants (no atomics, fixed order). */
long fabind_pair_bias_cat_parts(int B, int max_P);
int fabind_pair_bias_cat(const void* const* douts, int nblk, const int* desc_p, int B, int max_P, int Kp, void* Acat, int lda,
                         const float* b0, int ld_ab, const int* c_index, const float* wcomp, int H, void* BTcat, int ldb,
                         float* colpart, hipStream_t stream);
/* BTcat alone -- BTcat[b * H + h, k * Kp + j * 8 + o] = b0[c_index[lig0_b + j], h] * wcomp[k][o][h] (bf16, zero padded) -- for callers that
 * write the gradient rows Acat themselves (fabind_cross_attn_fused_bwd; pass wcomp rows in ITS slot order). */
int fabind_pair_bias_btcat(const float* b0, int ld_ab, const int* c_index, const int* desc_p, const float* wcomp, int nblk, int H, int Kp,
                           void* BTcat, int ldb, int B, hipStream_t stream);
/* Batched transpose with zero padding, bf16: for b < B, k < nsub, m < cols:
 *   out[(k*B + b)*cols + m][i] = in[desc[b][0] + i][k*cols + m]  for i < desc[b][1], 0 for i up to Pp   (out row stride Pp).
 * Turns the row-major per-complex operands of the pair-bias adjoint into the K-major, uniformly padded layout the pipelined NT GEMM
 * takes with plain groups. */
int fabind_batched_transpose_pad(const void* in, int ld_in, const int* desc, int B, int nsub, int cols, int Pp, void* out,
                                 hipStream_t stream);
int fabind_pair_hadamard_bwd(const void* dhd, int dt, int ldh, const float* a0, const float* b0, int ld0, int H,
                             const float* a1, const float* b1, int ld1, int H2, const int* red_p, const int* red_c, int n,
                             float* da0, float* db0, int ldd0, float* da1, float* db1, int ldd1, hipStream_t stream);
/* Adjoint of the pair Hadamard over the ALL-PAIRS list of a batch (pair (b, i, j) at pair_off[b] + i * C_b + j: FABind+ threads the
 * pair embedding over every protein x ligand pair, FABind_plus/fabind/models/model_utils.py:96-146) without float atomics: one wave per
 * node, one writer per element.  T = (a | b) fp32 rows; dT receives d a in columns [0, W) of protein rows and d b in [W, 2W) of ligand
 * rows.  node_b[n] = complex of node n; desc_p = the layout's int32[8] block descriptors (pair offset in words 4, 5). */
int fabind_pair_hadamard_bwd_grid(const void* dhd, int dt, int ldh, const float* T, int ldt, int W, const int* node_off,
                                  const int* c_cnt, const int* node_b, const int* desc_p, int n_nodes, float* dT, int lddt,
                                  hipStream_t stream);
/* Forward-only node-level chain over 64-row tiles with the hidden activation kept in LDS (csrc/node_chain.hip):
 *   kind 0: out = act([X1 | X2] W1^T + b1) W2^T + b2 (+ R)   hidden = H    -- MC_E_GCL.node_model, FABind/fabind/models/egnn.py:99-109
 *   kind 1: out = act(X1 W1^T + b1) W2^T + b2 (+ R)          hidden = 2 H  -- Transition, FABind/fabind/models/model_utils.py:162-175
 * X1, X2: bf16 [M, H]; every weight operand is one H x H block in the fragment order of the fused edge kernels ([K/32][N/16][64][8]):
 * kind 0: W1a / W1b = W1[:, :H] / W1[:, H:], W2a = W2 (W2b unused); kind 1: W1a / W1b = W1[:H] / W1[H:], W2a / W2b = W2[:, :H] / W2[:, H:].
 * b1 has the hidden width; R (optional) and out are fp32 [M, H]; out16 (optional) receives bf16(out).  act = FB_ACT_SILU | FB_ACT_RELU.
 * H in {128, 256, 512}. */
int fabind_node_chain_fwd(const void* X1, int ld1, const void* X2, int ld2, const void* W1a, const void* W1b, const float* b1,
                          const void* W2a, const void* W2b, const float* b2, int act, int kind, const float* R, int ldr, float* out,
                          int ldo, void* out16, int ldo16, int M, int H, hipStream_t stream);
/* The same chains in SPLIT PRECISION (round 6; bf16 mode with config.set_split_sites(3)): fp32 X rows and fp32 master weights given as
 * hi | lo bf16 fragment packs (hi = bf16(W), lo = bf16(W - hi), each in the layout of fabind_node_chain_fwd's packs); every product term
 * is three MFMAs, the hidden layer is never rounded to bf16.  X1 / X2 / R / out: fp32 rows (ld % 4 == 0, 16-byte aligned).
 * t16 (training forward; NULL otherwise): bf16 [M, hidden] of the activated hidden layer, d16 (SiLU only): bf16 of its derivative -- the
 * operands of the bf16 backward (weight gradient of the second Linear, activation adjoint inside the input-gradient GEMM). */
int fabind_node_chain_x3_fwd(const float* X1, int ld1, const float* X2, int ld2, const void* W1ah, const void* W1al, const void* W1bh,
                             const void* W1bl, const float* b1, const void* W2ah, const void* W2al, const void* W2bh, const void* W2bl,
                             const float* b2, int act, int kind, const float* R, int ldr, float* out, int ldo, void* out16, int ldo16,
                             void* t16, int ldt, void* d16, int ldd, int M, int H, hipStream_t stream);
/* Adjoint of out[e, :] = t[ia[e], :] * t[ib[e], :] (the distance-map head's LN(p_i) * LN(c_j) over every pocket residue x ligand atom
 * pair, FABind/fabind/models/model.py:355) without float atomics: the pairs of every row of t are given as a CSR (rowptr [n_rows + 1];
 * per entry the pair's row of dout and the partner's row of t); one wave per row, dT[n, :] = sum_e dout[pair_idx[e], :] * t[partner[e], :]
 * (written, not accumulated; rows without pairs receive zeros).  W <= 1024, W % 4 == 0.  Deterministic summation order. */
int fabind_rows_hadamard_bwd(const void* dout, int dt, int ldo, const float* t, int ldt, int W, const int* rowptr, const int* pair_idx,
                             const int* partner, int n_rows, float* dT, int lddt, hipStream_t stream);
/* fabind_pair_hadamard_bwd over the inter graph's reduced pairs without float atomics: one wave per node walks the inter edges of its own
 * row (pair = red_idx[e], partner = col[e]); t0 = (a | b) [N, 2H], t1 = (a | b) [N, 2 H2] (H2 may be 0), the sums are ADDED to d0 / d1
 * in the same layout.  Deterministic summation order. */
int fabind_pair_hadamard_bwd_rows(const void* dhd, int dt, int ldh, const float* t0, int ld0, int H, const float* t1, int ld1, int H2,
                                  const int* rowptr, const int* col, const int* red_idx, const int* red_c, int n_rows, float* d0,
                                  int ldd0, float* d1, int ldd1, hipStream_t stream);
int fabind_inter_attn_bwd(const float* qkv, int ldqkv, const float* cv, int ldcv, int H, const float* d,
                          const float* rhohat, const int* rowptr, const int* col, const int* mirror, const int* red_idx,
                          const float* w_rk, const float* w_rv, const float* wcr, const float* w3, const float* alpha,
                          const float* cvs, float clampv, int n_rows, const float* dh_out, const float* dx_out,
                          float* dqkv, float* dcv, float* dd, float* drh, float* dbias_red, float* dlogit, float* dcp,
                          float* wpart, int nblk, hipStream_t stream);
int fabind_inter_attn_bwd_rows(const float* qkv, int ldqkv, const float* cv, int ldcv, int H, const float* d,
                               const float* rhohat, const int* rowptr, const int* col, const int* mirror, const int* red_idx,
                               const float* w_rk, const float* w_rv, const float* wcr, const float* w3, const float* alpha,
                               const float* cvs, float clampv, int n_rows, const float* dh_out, const float* dx_out,
                               float* dqkv, float* dcv, float* dd, float* drh, float* dbias_red, float* dlogit, float* dcp,
                               float* wpart, int nblk, const int* order, int n_heavy, int n_act, hipStream_t stream);
int fabind_las_step_bwd(const float* x, const float* x0, const unsigned char* pass_mask, const int* las_i, const int* las_j,
                        const int* las_off, const int* node_off, const int* c_cnt, int B, int max_n, float step,
                        float clampv, const float* dout, float* dx, hipStream_t stream);
int fabind_pair_bias_bwd(const float* dout, int NO, const float* ab, int ld, int H, const float* w, const int* desc_p,
                         int B, int max_P, int max_C, const int* p_index, const int* c_index, float* dab, float* dwk,
                         hipStream_t stream);
/* dab[c_index[jc], H + h] += sum_o w[o,h] T[(jc,o),h];  dw_part[g * ld_part + o * H + h] = sum_{jc in group g of 16} ab[c_index[jc], H + h]
 * T[(jc,o),h] for g < fabind_pair_bias_finish_parts(n_c): per-group partials of the weight gradient, WRITTEN (no float atomics); the
 * caller sums the rows (fabind_colsum over [parts, ld_part]) -- several blocks' partials side by side take one sum. */
int fabind_pair_bias_finish_parts(int n_c);
int fabind_pair_bias_finish(const float* T, const float* ab, int ld, int H, const float* w, const int* c_index, int n_c,
                            float* dab, float* dw_part, long ld_part, hipStream_t stream);
void fabind_gemm_set_config(int cfg); /* development knob: tile configuration of the bf16 LDS-DMA GEMM (default 13 = 256x128x32, 3 stages,
                                         two work-groups per CU; 0 = register-staged kernel; 1-9 = other tiles; results do not depend on it) */
void fabind_gemm_set_persistent(int on); /* development knob: persistent tile walk for long-M/short-K GEMMs */
int fabind_gemm_x3_occupancy(int wm); /* development probe: resident work-groups per CU of the split-bf16 GEMM kernel (hipOccupancyMaxActiveBlocksPerMultiprocessor) */
void fabind_cross_attn_fused_set_dbg(void* five_int64_on_device); /* development probe: phase cycle counters of one work-group of the fused cross-attention forward (NULL = off) */
int fabind_cross_attn_fused_occupancy(int lds_bytes); /* the same for the fused cross-attention forward at the given dynamic LDS size */
void fabind_gemm_set_x3_tile(int wm); /* development knob: tile height of the split-bf16 fabind_gemm kernel in units of 64 rows (2 = default: 128x128, two 4-wave work-groups per CU; 4: 256x128, one 8-wave work-group) */
void fabind_gemm_set_small_m(int tiles); /* development knob: fabind_gemm launches with fewer 256x128 tiles than this use 128x128 tiles (default 100; 0 = never); results are bitwise equal */
void fabind_gemm_tn_set_waves(int waves); /* development knob: work-group layout of fabind_gemm_tn: 16 (default) = 256x256 tile, 8 waves, 4-stage ring; 20 = the same with 5 stages; 4 = 256x128 tile, 4 waves, two work-groups per CU; 8 = 256x128, 8 waves.  Results are bitwise equal for equal `splits` */
int fabind_gemm_tn_tile_n(void);          /* 256 or 128: columns of an output tile under the current layout (the host sizes `splits` from the tile count) */
void fabind_gemm_tn_set_exp(int mask);    /* probe knob (tools/probes/gemm_tn_bench.py): 1 = no operand loads after the pipeline fill, 4 = operand loads re-read the first rows (cache hits); 2 is retired (ignored); 0 in production */

#ifdef __cplusplus
}
#endif
#endif
