/*
 * phyloformer_amd — C ABI of the MI355X (gfx950) Phyloformer inference path.
 *
 * One shared library (libphyloformer_amd.so, built by hipcc for gfx950) owns
 * device memory, the HIP stream, the pre-split weights and every kernel.  The
 * Python host code (phyloformer_amd/engine.py) binds these symbols with
 * ctypes; nothing in the signatures is a torch / numpy type.
 *
 * What each entry point replaces in the reference (lucanest/Phyloformer; the
 * reference has no FFI layer of its own, its boundary is Python-level —
 * SURVEY.md §8b):
 *
 *   pf_create            Phyloformer(**hp) + load_state_dict + .to(device) + .eval()
 *                        infer_alns.py:71-86, phyloformer/model.py:109-164
 *   pf_forward           model(aln[None, :].float())
 *                        infer_alns.py:112 -> phyloformer/model.py:166-187
 *                        (embedding :173, pair expansion :175, 6 x PhyloformerLayer
 *                        :87-106 with ScaledLinearAttention attention.py:160-197,
 *                        pwFNN + Softplus :182, site mean :185)
 *   pf_forward_sharded   the same forward for a contiguous block of sites of every
 *                        pair; row-attention statistics (attention.py:183-190 with
 *                        dim=-2 = sites, model.py:91) and the final site sums
 *                        (model.py:185) are all-reduced over RCCL.  The reference has
 *                        no multi-device inference; this is the build's site-sharding.
 *   pf_destroy           garbage collection of the nn.Module
 *
 * Conventions
 *   - every function returns PF_OK (0) or a negative pf_status; nothing throws
 *     across the ABI; pf_last_error() gives the message for the last failure on
 *     that handle (or, with NULL, the last failure of pf_create on this thread);
 *   - the caller owns all host buffers; the library owns all device memory and
 *     copies the weights at pf_create;
 *   - a handle is bound to one device and one stream and is not thread-safe;
 *     distinct handles are independent;
 *   - residues are alphabet indices 0..21 in the order "ARNDCQEGHILKMFPSTWYVX-"
 *     (phyloformer/data.py:7); the one-hot tensor of the reference never exists;
 *   - pairs are enumerated (i, j), i < j, lexicographically (model.py:13-17),
 *     P = N(N-1)/2 outputs per alignment.
 *
 * Sections and bindings
 *   - a comment that opens with four dashes is a section banner; a function belongs to the last banner above it (the
 *     functions above the first banner to none);
 *   - a function may be missing from a library of this PF_ABI_VERSION if and only if its banner says
 *     "(additive to ABI n)": a binding resolves such a function when it is called, every other one when the library is
 *     loaded.  A function added without a new ABI version goes under a banner that says so;
 *   - phyloformer_amd/cabi.py reads the prototypes, this rule, pf_status and the #defines from this file: a prototype
 *     is written with its return type and name on one line, in the types int, int32_t, int64_t, uint64_t, size_t, void
 *     and pointers.
 */
#ifndef PHYLOFORMER_AMD_H
#define PHYLOFORMER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_ABI_VERSION 5

typedef enum pf_status {
    PF_OK = 0,
    PF_EINVAL = -1,  /* bad dims, residue index > 21, N > max_seqs, unsupported architecture */
    PF_EHIP = -2,    /* a HIP runtime call or kernel launch failed */
    PF_ERCCL = -3,   /* RCCL missing or a collective failed */
    PF_ENOMEM = -4,  /* device or host allocation failed */
    PF_ESTATE = -5,  /* call not valid in the handle's current state */
    PF_EIO = -6      /* a file could not be read (pf_fasta_batch_load: detail = errno) */
} pf_status;

/* Flat fp32 weight blob.  Order (phyloformer_amd/weights.py::blob_layout):
 *   embedding_block.0.weight [E][22], .bias [E];
 *   per block b, for a in (row, col):
 *       a_norm.weight [E], a_norm.bias [E],
 *       q_proj.weight [H][E], q_proj.bias [H], k_proj.weight [H][E], k_proj.bias [H],
 *       v_proj.weight [E][E], v_proj.bias [E], out_proj.weight [E][E], out_proj.bias [E];
 *     then ffn_norm.weight [E], ffn_norm.bias [E],
 *       ffn.0.weight [4E][E], ffn.0.bias [4E], ffn.3.weight [E][4E], ffn.3.bias [E];
 *   pwFNN.0.weight [E], pwFNN.0.bias [1].
 * Supported: n_alphabet 22, 1 <= n_blocks <= 64, 1 <= E <= 256 and E divisible by H (the reference's own
 * rule); the FFN width is 4 E.  E = 64, H = 4 (all shipped checkpoints) runs on the default kernels; every other
 * architecture on the generic float64 kernels (option "generic").  Anything else is refused with PF_EINVAL. */
typedef struct pf_weights_t {
    int32_t n_blocks;
    int32_t n_heads;
    int32_t embed_dim;
    int32_t n_alphabet;     /* 22 */
    const float* blob;
    uint64_t blob_len;      /* number of floats */
} pf_weights_t;

typedef struct pf_handle pf_handle_t;

/* Expected blob_len for an architecture, so bindings can check before calling. */
uint64_t pf_blob_len(int32_t n_blocks, int32_t n_heads, int32_t embed_dim);

int pf_abi_version(void);

/* What this library was built from (ABI 4): a JSON object, static storage -
 *   {"abi", "arch", "hipcc" (HIP and clang versions), "sched_strategy" ("iterative-ilp" | "default"),
 *    "sched_fallback" (true when hipcc could not compile pf_lib.hip with the intended strategy and
 *    phyloformer_amd/build.py was allowed to fall back: 1-7 % slower kernels), "flags" per translation unit,
 *    "source_hash" (sha256/16 over csrc/ + include/), "kernel_hash" (pf_device.hip.h + the flags of its unit)}.
 * bench.py copies it into its line and refuses PMC traffic figures taken with another kernel_hash. */
const char* pf_build_info(void);

/* Create a handle on HIP device `device`: uploads the weights, builds the
 * embedding table and the fp16 hi/lo MFMA operand images.  Fails with PF_EHIP
 * if no gfx950 device is present: there is no CPU fallback.
 * An architecture outside the supported set (pf_weights_t) fails with PF_EINVAL before any device access
 * ("embed_dim must be 1..256 and divisible by n_heads").  For E = 64, H = 4 the default and float64 "precise"
 * images are built (the generic image waits for the first forward with option "generic" = 1); for any other
 * supported architecture only the generic float64 image (csrc/pf_generic.hip.h) is built, and every forward entry
 * point runs on the generic kernels. */
int pf_create(const pf_weights_t* w, int device, pf_handle_t** out);
int pf_destroy(pf_handle_t* h);
const char* pf_last_error(const pf_handle_t* h);

/* Options (before or between forwards):
 *   "max_seqs"   int   sequence cap, default 200 (model.py:39); 0 lifts it
 *   "profile"    int   1 = bracket every launch with HIP events (see pf_profile_*); 2 = only the
 *                      dominant kernel k_main (event pairs serialise the stream: 1 costs ~15 %, 2 ~5 %)
 *   "debug_keep" int   1 = keep per-layer activations for pf_debug_read
 *   "force_rccl" int   1 = pf_comm_init creates a real RCCL communicator even for one rank (tests)
 *   "ws_limit_mb" int  workspace budget per batch chunk (default 24576)
 *   "sub_floats" int   distances one sub-call of pf_forward_leave_one_out / pf_forward_place / pf_forward_tiled may
 *                      hold on the device (default 4194304; <= 0 restores it); sub-calls are whole sources, one source
 *                      always runs whole, and the results do not depend on it; tests/tuning
 *   "spr_pairs_simple" int 1 = pf_bme_spr forms its pair table with the one-thread-per-entry kernel instead of the
 *                      tiled one (default 0): the same bits; the baseline of tools/spr_bench.py
 *   "delta_atomic" int 0 = pf_delta evaluates every quartet six times, once for each of its pairs, without atomics
 *                      on the pair sums, instead of once with LDS and global atomics (default 1): the same integers;
 *                      the comparison of tools/delta_bench.py
 *   "fit_lds_bytes" int bytes of LDS in which pf_tree_fit's pair kernel may stage a tree's node arrays (12 bytes a node);
 *                      <= 0 (default): the 163,840 of a CU, N <= 6,827; a tree above it is read from global memory: the
 *                      same bits; tests
 *   "spr_step_cap" int moves after which pf_bme_spr caps a source (status 2); <= 0 (default): 16 N; tests
 *   "colstats_fine" int k_colstats blocks per pair group (0), per run of a group (1) or chosen from the batch
 *                      size (-1, default): the same summation tree either way, so the same bits; tests/tools
 *   "two_streams" int  0 = a batch runs on one stream; default 1: forwards of >= 2 alignments run as two
 *                      independent half-batches on two streams (same results bit for bit, a few % faster);
 *                      environment PF_TWO_STREAMS=0/1 sets the initial value (A/B runs of whole programs)
 *   "overlap"    int   0 = site-sharded forwards issue one collective per block for the whole batch instead of
 *                      two half-batches on two streams
 *   "reserve_cus" int  CUs the persistent kernels leave to the RCCL kernels while collectives run (default 8)
 *   "materialize_x0" int 1 = k_embed writes x0 = T[a_i] + T[a_j] to HBM and block 0 reads it (round-1 path);
 *                      default 0: block 0's kernels form it from the embedding table on the fly
 *   "embed_mfma" int   1 = compute block 0's row statistics with the MFMA kernel (k_main<FIRST>) instead of
 *                      the residue-pair table lookup (k_embed); cross-check only, same results to fp32 noise
 *   "precise"    int   which alignments take the float64 path (csrc/pf_precise.hip.h): -1 (default) = chosen from
 *                      the alignment's shape (fewer than 32 sites or 8,192 pair-site tokens: the distance is a mean over sites, and on a
 *                      handful of them the fp32 reference itself is 3e-5 ... 8e-4 from its float64 evaluation, so no
 *                      fp32-level kernel can promise 1e-4 against it), 0 = never, 1 = always (any shape in float64;
 *                      3-9 x slower).  The choice never depends on the batch.  Above the option: a checkpoint or
 *                      shape whose operands could overflow the default kernels' fp16 MFMA operands (weights ~ 1000 x
 *                      the trained ones, more than 2^20 sites) always runs in float64.
 *   "recheck_above" int  range re-check of pf_forward / pf_forward_sharded (the host-buffer entry points; only while
 *                      "precise" is -1): an alignment whose largest predicted distance exceeds this many substitutions
 *                      per site (default 8; 0 = off), or is not finite, is computed again on the float64 kernels before
 *                      the call returns.  An absolute tolerance of 1e-4 on a value of 10 asks for 1e-5 relative - the
 *                      rounding level of fp32 arithmetic itself, the reference's included; alignments stay far below
 *                      (<= 5 on the reference's test data), uniformly random residues do not (9-13).  Per alignment,
 *                      never a function of the batch; pf_profile_get("rechecked") counts them.  The device entry
 *                      points do not re-check (their results never pass through the host).
 *   "generic"    int   the generic float64 kernels (csrc/pf_generic.hip.h: any embed_dim / n_heads, reference op order,
 *                      fp64 matrix cores).  On an E = 64, H = 4 handle: 0 (default) = the routing above, 1 = every
 *                      forward on the generic kernels (cross-check against the shipped checkpoints; the image is built
 *                      on the first such forward).  On any other handle they are the only path: 1 is accepted, 0 is
 *                      refused with PF_EINVAL, and "precise" / "recheck_above" are accepted but have no effect (float64
 *                      throughout needs neither).  Site-sharded runs issue n_blocks + 1 float64 all-reduces on one
 *                      stream; batches are chunked under "ws_limit_mb"; pf_profile_get("generic") counts the launches.
 *   "site_dedup" int   default 1: the column statistics of the default kernels are computed once per DISTINCT alignment
 *                      column (k_site_classes finds the classes of equal columns at the start of every forward, sharded,
 *                      weighted, site-table, taxon, placement and tiled ones included) and read for its repeats: no sum
 *                      changes its order, the results are the same bits.  0 = every site is its own class (the same
 *                      kernels over the identity map; A/B runs).  pf_site_classes returns the classes.
 *   "main_dedup" int   default 1: an alignment with enough repeated columns (k_site_classes; the share is measured,
 *                      DESIGN.md section 9) runs every block's row apply, column apply and feed-forward once per DISTINCT
 *                      column: a compact k_main launch over the first sites, then the row statistics (the head: its site
 *                      sums) over every site in place, so no sum changes its order - the results are the same bits.  The
 *                      route is decided per alignment on the device, from the alignment's own columns.  0 = every
 *                      alignment through the fused launch; 2 = every alignment through the split route, even one without a
 *                      repeat (tests).  Site-sharded and emulated ranks route from the classes of their own site range.
 *                      Weighted and site-map forwards, "embed_mfma" and "materialize_x0" stay on the fused launch.
 *   "stats_dedup" int  default 1: the row statistics of an alignment on the split route ("main_dedup") are formed once per
 *                      DISTINCT column of a pair row as well - v, q' and k' per distinct token into an on-chip table, then
 *                      every site reduced in place, in the lanes and partial slots of the original tiling (k_row_stats): no
 *                      sum changes its order, the results are the same bits.  Alignments with more distinct columns than
 *                      the table holds (ROW_STATS_KMAX, csrc/pf_layout.h) keep the statistics launch; the choice is made
 *                      per alignment on the device.  0 = every split alignment through the statistics launch (A/B runs).
 * Test / tool switches, not part of the contract:
 *   "colstats_ring" int  0 = k_colstats prefetches its rows through registers instead of the per-wave LDS ring (the
 *                      same bits; A/B and counter runs)
 *   "precise_ffn_valu" int 1 = the float64 FFN on the plain VALU kernel instead of the fp64 matrix cores (cross-check)
 *   "phase_prof"  int  1 = in-kernel phase timers of k_main (pf_debug_read "phase_prof"); 2 = of the last
 *                      block's launch only
 *   "head_fold"   int  default 1: the last block's FFN output projection is folded into the softplus head (one dot
 *                      product per token instead of the 256 -> 64 GEMM); 0 = the full last FFN (cross-check).
 *                      With debug_keep = 1 the full last FFN runs as well, for the "x<n_blocks>" tap only
 *   "ablate"      int  energy experiments: phases of k_main switched off - RESULTS INVALID
 */
int pf_set_option(pf_handle_t* h, const char* key, int64_t value);

/* Forward pass.  idx: host uint8 [B][N][L]; out: host float [B][P].
 * Synchronous: returns after `out` is filled (and re-checked, option "recheck_above").  Never communicates: on a handle that carries a
 * communicator (pf_comm_init) pf_forward / pf_forward_device still process this rank's own
 * alignments only (alignment-level data parallelism); collectives belong to pf_forward_sharded*.
 * Errors: PF_EINVAL for B < 1, N < 2, L < 1, N > max_seqs, or an index > 21. */
int pf_forward(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, float* out);

/* Same with device-resident buffers, asynchronous on the handle's stream
 * (used by the benchmark so the timed region starts with inputs in HBM).
 * d_idx: device uint8 [B][N][L]; d_out: device float [B][P].
 * Residues are NOT validated on this path (the bytes never pass through the host).  A byte > 21 cannot
 * fault: every table lookup of the kernels clamps it to 21 ('-').  It is reported late: the embedding
 * kernel raises a sticky flag on the handle, and the next pf_synchronize / pf_memcpy_d2h on it returns
 * PF_EINVAL once (the results of the forwards since the previous synchronisation are then those of the
 * clamped alignment, not of a valid one).  pf_forward / pf_forward_sharded keep refusing such input up
 * front (the reference raises KeyError, phyloformer/data.py:25-26). */
int pf_forward_device(pf_handle_t* h, const uint8_t* d_idx, int32_t B, int32_t N, int32_t L,
                      float* d_out);

/* ---- Felsenstein's bootstrap over alignment sites (additive to ABI 5) ------------------------------
 *
 * The replicate stream: replicate r (0-based) of an alignment of L sites takes, at output position l, the source site
 *   mix64(z) = SplitMix64's finaliser (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
 *              z ^= z >> 31, mod 2^64);  key = mix64(seed + 0x9E3779B97F4A7C15);
 *   site = ((mix64(key ^ ((r << 32) | l)) >> 32) * L) >> 32.
 * It depends on (seed, r, l, L) only (phyloformer_amd/bootstrap.py::resample_sites is its host twin). */
/* d_src uint8 [B][N][L] -> d_dst uint8 [B][R][N][L], replicates r_begin .. r_begin+R-1 of the stream above; async. */
int pf_resample_sites_device(pf_handle_t* h, const uint8_t* d_src, int32_t B, int32_t N, int32_t L,
                             int32_t r_begin, int32_t R, uint64_t seed, uint8_t* d_dst);
/* idx host uint8 [B][N][L] -> out host float [B][R][P]: the distances of R bootstrap replicates of every alignment.
 * Synchronous.  out[b][r] equals, bit for bit, pf_forward of the host-resampled replicate r of idx[b], on the path
 * pf_forward would take (options "precise", "generic", "ws_limit_mb", "max_seqs" and the range re-check
 * "recheck_above" per replicate included) for any B, R and chunking.  The sources are uploaded once; replicate bytes
 * are built on the device one forward chunk at a time.  Validated before any device work, with pf_forward's
 * messages, plus R >= 1 and no size_t overflow of B*R*P or B*R*N*L.  Never communicates. */
int pf_bootstrap(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, int32_t R,
                 uint64_t seed, float* out);

/* ---- derived alignments as lists of source sites: site tables and window scans (additive to ABI 5) ----
 *
 * A derived alignment is a list of K source sites of an alignment of L sites; S of them per source, all of one K (a
 * forward launch needs one shape).  Two maps:
 *   table   set s takes sites[s][l], l = 0..K-1: any indices in [0, L), repeats and any order allowed;
 *   affine  set s takes start[s] + l: a window of K consecutive sites.
 * The window rule (phyloformer_amd/windows.py::window_starts is its host twin): windows of W sites start at
 * 0, step, 2 step, ... while start + W <= L; if the last of them ends before L, one more window is anchored at L - W,
 * so that every site is covered.  W == L gives one window. */
/* Number of windows, and the first site (0-based) of window s; PF_EINVAL for W < 1, W > L, step < 1 or s outside
 * [0, pf_window_count).  No handle, no GPU. */
int pf_window_count(int32_t L, int32_t W, int32_t step);
int pf_window_start(int32_t L, int32_t W, int32_t step, int32_t s);
/* d_src uint8 [B][N][L] -> d_dst uint8 [B][S][N][K] (k_gather_sites, csrc/pf_sites.hip.h); async on the handle's
 * stream.  Exactly one of d_sites (device int32 [S][K], table) and d_start (device int32 [S], affine) is not NULL;
 * 1 <= K <= L.  The map never passes through the host, so it is not validated here: an entry outside [0, L) (a start
 * outside [0, L - K]) is never dereferenced - site 0 is read in its place - and is reported late, like a residue > 21
 * of pf_forward_device: the next pf_synchronize / pf_memcpy_d2h on the handle returns PF_EINVAL once. */
int pf_gather_sites_device(pf_handle_t* h, const uint8_t* d_src, int32_t B, int32_t N, int32_t L, const int32_t* d_sites,
                           const int32_t* d_start, int32_t S, int32_t K, uint8_t* d_dst);
/* idx host uint8 [B][N][L], sites host int32 [S][K] -> out host float [B][S][P].  Synchronous.  out[b][s] equals, bit
 * for bit, pf_forward of the host-cut alignment idx[b][:, sites[s]], on the path pf_forward would take for shape (N, K)
 * (the float64 route for K < 32 or fewer than 8,192 pair-site tokens; options "precise", "generic", "ws_limit_mb",
 * "max_seqs" and the range re-check "recheck_above" per derived alignment included) for any B, S and chunking.  The
 * sources are uploaded once; derived bytes are built on the device one forward chunk at a time and never exceed one
 * chunk.  Validated before any device work, with pf_forward's messages where they apply: 1 <= K <= L, S >= 1, every
 * table entry in [0, L) (refused, never clamped), no size_t overflow of B*S*P or B*S*N*K, and everything pf_forward
 * checks (residues > 21 included); every failure is PF_EINVAL and leaves `out` untouched.  Never communicates. */
int pf_forward_sites(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, const int32_t* sites, int32_t S,
                     int32_t K, float* out);
/* The same for the S = pf_window_count(L, W, step) windows of the rule above (K = W): out host float [B][S][P] holds
 * S_cap windows per source; step < 1, W outside [1, L] and S_cap < S are PF_EINVAL. */
int pf_forward_windows(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, int32_t W, int32_t step,
                       float* out, int32_t S_cap);

/* ---- derived alignments as lists of source rows: taxon subsets and leave-one-out (additive to ABI 5) ----
 *
 * A derived alignment is a list of M source rows of an alignment of N sequences, all L sites; S of them per source,
 * all of one M (a forward launch needs one shape).  Set s takes the rows taxa[s][m], m = 0..M-1: any rows in [0, N),
 * repeats and any order allowed, M may exceed N.  Phyloformer's distances are context dependent - column attention
 * mixes all pairs - so the distance between two sequences changes when a third leaves the alignment; these calls
 * compute that from one upload of the sources.
 * Pair order everywhere: the reference's, the row-major upper triangle - pair (i, j), i < j, of N rows has index
 * i (2N - i - 1) / 2 + (j - i - 1).  Leave-one-out set t is the alignment without row t, the remaining rows in order:
 * pair (i, j), neither of them t, has there the index of (i - (i > t), j - (j > t)) among N - 1 rows. */
/* d_src uint8 [B][N][L] -> d_dst uint8 [B][S][M][L] (k_gather_taxa, csrc/pf_taxa.hip.h), d_taxa device int32 [S][M], the
 * same table for all B sources; async on the handle's stream.  The table never passes through the host, so it is not
 * validated here: an entry outside [0, N) is never dereferenced - row 0 is read in its place - and is reported late,
 * like pf_gather_sites_device's: the next pf_synchronize / pf_memcpy_d2h on the handle returns PF_EINVAL once. */
int pf_gather_taxa_device(pf_handle_t* h, const uint8_t* d_src, int32_t B, int32_t N, int32_t L, const int32_t* d_taxa,
                          int32_t S, int32_t M, uint8_t* d_dst);
/* idx host uint8 [B][N][L], taxa host int32 [S][M] -> out host float [B][S][M (M - 1) / 2].  Synchronous.  out[b][s]
 * equals, bit for bit, pf_forward of the host-cut alignment idx[b][taxa[s], :], on the path pf_forward would take for
 * shape (M, L) (options "precise", "generic", "ws_limit_mb", "max_seqs" and the range re-check "recheck_above" per
 * derived alignment included) for any B, S and chunking.  The sources are uploaded once; derived bytes are built on the
 * device one forward chunk at a time.  Refused before any device work, `out` untouched: everything pf_forward checks, at
 * shape (M, L) as well as (N, L) (residues > 21 included); S < 1; M < 2; a table entry outside [0, N) (refused, never
 * clamped; the message names set and position); NULL buffers; sizes that overflow size_t; and (PF_ESTATE) a handle
 * whose communicator has more than one rank.  Never communicates. */
int pf_forward_taxa(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, const int32_t* taxa, int32_t S,
                    int32_t M, float* out);
/* Leave-one-out taxon influence.  idx host uint8 [B][N][L], N >= 3.  Synchronous.  With P = N (N - 1) / 2 and
 * P1 = (N - 1)(N - 2) / 2:
 *   out       float [B][P]       pf_forward's result, bit for bit
 *   loo       float [B][N][P1]   (may be NULL) loo[b][t] = pf_forward_taxa of the set "all rows but t", bit for bit
 *   and, with delta_t(i, j) = loo[t][index of (i, j) in set t] - out[(i, j)] (exact in double),
 *   influence float [B][N]       sqrt( mean over the P1 pairs of delta_t^2 ): how far removing t moves the others
 *   shift     float [B][N]       mean over the P1 pairs of delta_t: signed - did t's presence stretch or shrink them
 *   context   float [B][P]       sqrt( sum_{t != i, j} delta_t(i, j)^2 / (N - 2) ): how much a distance depends on who
 *                                else is in the alignment
 * The statistics are reduced on the device after the range re-check has replaced flagged sets, in double, rounded to
 * float once, no atomics: their bits are a function of (N, out, loo) only, batch invariant.  They are descriptive, not
 * a test statistic.  The N cuts of every source run through the same driver as pf_forward_taxa, in sub-calls, so
 * that loo on the device never exceeds one sub-call.  Refusals as pf_forward_taxa's, plus N < 3. */
int pf_forward_leave_one_out(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, float* out, float* loo,
                             float* influence, float* shift, float* context);
/* The reduction alone (k_loo_taxon, k_loo_pair) on device arrays d_full float [B][P], d_loo float [B][N][P1] ->
 * d_influence [B][N], d_shift [B][N], d_context [B][P]; async on the handle's stream.  B >= 1, N >= 3. */
int pf_loo_stats_device(pf_handle_t* h, const float* d_full, const float* d_loo, int32_t B, int32_t N, float* d_influence,
                        float* d_shift, float* d_context);

/* ---- query placement: distances of added sequences to a backbone (additive to ABI 5) ----
 *
 * "Add one in", the mirror of leave-one-out.  An alignment of M sequences is a backbone - its first N = M - Q rows,
 * N >= 2 - followed by Q >= 1 queries, where `mafft --add` and its kin put them.  Distances are context dependent, so a
 * query's distances to the backbone change with whichever other queries share its forward: every query is therefore
 * forwarded alone with the backbone.  Set q is the rows (0, .., N - 1, N + q), in that order: the query is its row N.
 * With P_n = n (n - 1) / 2 and pair_n(i, j) the pair order above among n rows:
 *   out     float [B][P_M]           pf_forward(idx), bit for bit
 *   base    float [B][P_N]           pf_forward of rows 0 .. N - 1, bit for bit
 *   sets    float [B][Q][P_{N+1}]    (may be NULL) sets[b][q] = pf_forward_taxa of (0, .., N - 1, N + q), bit for bit
 *   place   float [B][Q][N]          place[q][i] = sets[q][pair_{N+1}(i, N)]: query q's distance to backbone row i (a copy)
 *   and, with delta_q(i, j) = sets[q][pair_{N+1}(i, j)] - base[pair_N(i, j)] over the P_N backbone pairs (exact in double),
 *   disturb float [B][Q]             sqrt( mean delta_q^2 ): how far the query's presence moves the backbone's own distances
 *   shift   float [B][Q]             mean delta_q: signed
 *   joint   float [B][Q]             sqrt( mean_i (out[pair_M(i, N + q)] - place[q][i])^2 ): how far the OTHER queries'
 *                                    presence moves q's distances to the backbone (0 when Q = 1 up to the forward's bits)
 * Synchronous; the sources are uploaded once; never communicates.  The whole, the backbone and the Q sets each take
 * the path pf_forward would take for their own shapes (M, L), (N, L), (N + 1, L) (options "precise", "generic",
 * "ws_limit_mb", "max_seqs" and the range re-check per derived alignment included).  The statistics are reduced on the
 * device after the range re-check has replaced flagged sets, in double, rounded to float once, no atomics: their bits
 * are a function of (N, Q, out, base, sets) only, batch invariant.  They are descriptive, not a test statistic.  The
 * sets run in sub-calls, so that `sets` on the device never exceeds one sub-call.  Refused before any device work,
 * every output untouched: everything pf_forward checks, at all three shapes (residues > 21 included); Q < 1; M - Q < 2;
 * NULL buffers other than sets; sizes that overflow size_t; and (PF_ESTATE) a handle whose communicator has more than
 * one rank. */
int pf_forward_place(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t M, int32_t L, int32_t Q, float* out, float* base,
                     float* sets, float* place, float* disturb, float* shift, float* joint);
/* The reduction alone (k_place_rows, k_place_backbone; csrc/pf_place.hip.h) on device arrays d_whole float [B][P_{N+Q}],
 * d_base float [B][P_N], d_sets float [B][Q][P_{N+1}] -> d_place [B][Q][N], d_disturb, d_shift, d_joint [B][Q]; async on
 * the handle's stream.  B >= 1, N >= 2, Q >= 1. */
int pf_place_stats_device(pf_handle_t* h, const float* d_whole, const float* d_base, const float* d_sets, int32_t B, int32_t N,
                          int32_t Q, float* d_place, float* d_disturb, float* d_shift, float* d_joint);

/* ---- tiled inference: alignments beyond the sequence cap (additive to ABI 5) ----
 *
 * A forward holds P L 64 floats of residual stream and the checkpoints were trained on a few tens of sequences, so an
 * alignment of N sequences beyond "max_seqs" is not forwarded whole: it is covered by sets of at most M rows - the
 * CONTEXT a distance is predicted in, which is part of its definition (distances are context dependent).  The plan
 * (csrc/pf_tile_host.h; phyloformer_amd/tile.py::plan is the Python twin), for 2 <= M and N > M:
 *   G = ceil(N / floor(M / 2)) groups, G >= 3; group g is the contiguous rows [floor(g N / G), floor((g + 1) N / G)):
 *   sizes differ by at most one.  Set (g, h), g < h, in lexicographic order, is the rows of group g followed by the rows
 *   of group h: m = n_g + n_h <= M rows, S = G (G - 1) / 2 sets of at most three distinct sizes.  A cross-group pair
 *   lies in exactly one set; a within-group pair of group g in the G - 1 sets that contain g.
 * The sets' token count is about 2 (G - 1) / G times that of the untiled forward; memory stays that of one forward chunk.
 *   out    float [B][P_N]   cross-group pair: its one value, the bits of pf_forward_taxa of its set.  Within-group
 *                           pair: the mean of its G - 1 values, added in double in ascending order of the partner
 *                           group, divided and rounded to float once.
 *   spread float [B][P_N]   within-group pair: sqrt( sum (d - mean)^2 / (G - 2) ) over those values, in double from the
 *                           unrounded mean: the standard deviation of the distance over its contexts.  Cross-group
 *                           pair: exactly 0 - ONE context, so no spread is measured; 0 does not mean "certain".
 *                           Descriptive, not a test statistic.
 * Synchronous; the sources are uploaded once; every set takes the path pf_forward takes for its own shape (m, L)
 * (options "precise", "generic", "ws_limit_mb" and the range re-check per set included); the sets' distances are
 * combined on the device (k_tile_combine, csrc/pf_tile.hip.h: no atomics, the bits are a function of (N, M, values)
 * only, batch invariant), in sub-calls of whole sources.  "max_seqs" is checked against M and every set size, NOT
 * against N.  Refused with PF_EINVAL before any device work, out and spread untouched: M < 2; M > max_seqs while the cap
 * is on (pf_forward's message); N <= M (call pf_forward); B < 1, L < 1; residues > 21; NULL buffers; sizes that overflow
 * size_t, or P_N >= 2^31.  PF_ESTATE: a handle whose communicator has more than one rank.  Never communicates. */
int pf_forward_tiled(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, int32_t M, float* out, float* spread);
/* The combination alone on device arrays: d_sets float [B][T] - the distances of the S sets of every source in (g, h)
 * order, each set's m (m - 1) / 2 distances in the pair order above, T their sum - -> d_out, d_spread float [B][P_N];
 * async on the handle's stream (the plan's tables are rebuilt, behind a synchronisation, only when (N, M) changes). */
int pf_tile_combine_device(pf_handle_t* h, const float* d_sets, int32_t B, int32_t N, int32_t M, float* d_out, float* d_spread);
/* The plan's numbers: G, and the first row of group g (0 <= g <= G; g = G gives N); PF_EINVAL for M < 2, N <= M or g
 * outside [0, G].  No handle, no GPU. */
int pf_tile_groups(int32_t N, int32_t M);
int pf_tile_bound(int32_t N, int32_t M, int32_t g);

/* ---- neighbour joining on the device: trees beyond the sequence cap (additive to ABI 5) ----
 *
 * The join sequence of neighbour joining (phyloformer_amd/nj.py::nj_joins; pf_nj_newick_n's nj_core is its host twin)
 * computed on the GPU, bit for bit: the symmetric double matrix of preds (pf_nj_newick_n's), numpy's pairwise row sums
 * of the active sub-matrix, q = ((m - 2) d_ab - r_a) - r_b without FMA, its first minimum in row-major order, the branch
 * lengths and the new node's distances - every float64 operation with the operands and in the order of the host code
 * (csrc/pf_nj.hip.h, csrc/pf_nj_host.h).  3 (N - 3) + 2 launches per call on the handle's stream,
 * no copy to the host and no synchronisation between them.  One call with B sources equals B calls with one.
 *   preds     float  [B][P_N]            pairs i < j in lexicographic order (pf_forward's output)
 *   slots     int32  [B][2 (N - 3) + 3]  a, b of every join (slot a < slot b; the new cluster takes slot a), then the
 *                                        three slots i, j, k of the trifurcation
 *   lengths   double [B][2 (N - 3) + 3]  la, lb of every join, then li, lj, lk
 *   nonfinite uint8  [B]                 1: the source holds a NaN or an infinity; its slots and lengths are UNSPECIFIED
 *                                        (the payload of a NaN made on the device is not the host's: run pf_nj_newick_n
 *                                        for such a source); 0: finite input, the table is nj_joins' bit for bit
 * pf_nj_joins takes host arrays and is synchronous; pf_nj_joins_device takes device arrays and is asynchronous on the
 * handle's stream.  The state is B N^2 doubles: sources run side by side in chunks that fit "ws_limit_mb"; one source
 * always runs whole.  Refused with PF_EINVAL before any device work: N < 3, B < 1; NULL buffers; P_N >= 2^31; an N whose
 * N^2 doubles alone exceed "ws_limit_mb" (the message names the bytes).  pf_profile_get("nj_joins") counts the calls. */
int pf_nj_joins(pf_handle_t* h, const float* preds, int32_t B, int32_t N, int32_t* slots, double* lengths, uint8_t* nonfinite);
int pf_nj_joins_device(pf_handle_t* h, const float* d_preds, int32_t B, int32_t N, int32_t* d_slots, double* d_lengths,
                       uint8_t* d_nonfinite);

/* ---- BIONJ on the device: FastME's default start tree (additive to ABI 5) ----
 *
 * The join sequence of BIONJ (Gascuel 1997; phyloformer_amd/bionj.py::bionj_joins states it) computed on the GPU, bit
 * for bit: neighbour joining with a matrix of variances beside the distances and one weight lambda per join.  The pair
 * of a join is the first of the scan (1,0), (2,0), (2,1), (3,0), ... of active positions whose q lies within 1e-9 of the
 * exact minimum; the joined cluster takes the row of the later position; lambda's sum is numpy's pairwise sum over the
 * active positions, by one thread (csrc/pf_bionj.hip.h, csrc/pf_bionj_host.h).  4 (N - 3) + 2
 * launches per call on the handle's stream, no copy to the host and no synchronisation between them.
 * Signatures, layouts and the meaning of nonfinite are pf_nj_joins': the table names a cluster by its smallest
 * sequence (slot a < slot b; the new cluster takes slot a), so pf_nj_format_joins_n, pf_bme_nni, pf_bme_spr,
 * pf_join_supports and pf_consensus_joins take it unchanged.  pf_bionj_joins takes host arrays and is synchronous;
 * pf_bionj_joins_device takes device arrays and is asynchronous on the handle's stream; pf_bionj_joins_host runs the
 * same kernel bodies serially without a handle or a device (a non-finite source's table is zeros there).  The state is
 * 2 B N^2 doubles: sources run side by side in chunks that fit "ws_limit_mb"; one source always runs whole.  Refused
 * with PF_EINVAL before any device work: N < 3, B < 1; NULL buffers; P_N >= 2^31; an N whose 2 N^2 doubles alone exceed
 * "ws_limit_mb" (the message names the bytes).  pf_profile_get("bionj_joins") counts the calls of the two handle entry
 * points. */
int pf_bionj_joins(pf_handle_t* h, const float* preds, int32_t B, int32_t N, int32_t* slots, double* lengths, uint8_t* nonfinite);
int pf_bionj_joins_device(pf_handle_t* h, const float* d_preds, int32_t B, int32_t N, int32_t* d_slots, double* d_lengths,
                          uint8_t* d_nonfinite);
int pf_bionj_joins_host(const float* preds, int32_t B, int32_t N, int32_t* slots, double* lengths, uint8_t* nonfinite);

/* ---- delta scores: how tree-like the distances are (additive to ABI 5) ----
 *
 * The delta plot of Holland, Huber, Dress & Moulton (2002; delta.plot of R's ape) of every source, bit for bit that of
 * phyloformer_amd/delta.py::delta_py.  For every quartet a < b < c < d of a source's N sequences: the three float64
 * sums d_ab + d_cd, d_ac + d_bd, d_ad + d_bc of float32 distances, ordered m1 >= m2 >= m3 by comparisons; delta =
 * (m1 - m2) / (m1 - m3), 0 where m1 == m3 (one correctly rounded float64 division); q = rint(delta 2^30), ties to even,
 * an integer in [0, 2^30].  A tree's distances give 0 for every quartet.  Everything behind q is integer arithmetic, so
 * no order of summation shows (csrc/pf_delta.hip.h, csrc/pf_delta_host.h).
 *   preds     float  [B][P_N]   pf_forward's distances, pairs i < j in lexicographic order
 *   pair_sum  int64  [B][P_N]   for the pair (i, j): the sum of q over the C(N - 2, 2) quartets that hold both.  The sum
 *                               over the pairs of sequence i is 3 times the sum of q over the quartets that hold i, the
 *                               sum over all pairs 6 times the sum over all quartets
 *   hist      int64  [B][K]     the quartets with min(K - 1, (q K) >> 30) equal to the bin, each counted once
 *   nonfinite uint8  [B]        1: the source holds a NaN or an infinity; its pair_sum and hist are zeros
 * pf_delta takes host arrays and is synchronous; pf_delta_device takes device arrays and is asynchronous on the
 * handle's stream; pf_delta_host visits every quartet once, serially, without a handle or a device.  One call with B
 * sources equals B calls with one.  The device evaluates every quartet once and adds its q to its six pairs by
 * integer atomics (option "delta_atomic"); it keeps no state per source; a call's work is cut into launches of a
 * bounded number of quartet evaluations, all on the handle's stream with no synchronisation between them.  Refused with
 * PF_EINVAL before any device work, the message naming the value: N < 4 or N > 2,048 (3 C(N - 1, 3) 2^30 must stay below
 * 2^63); B < 1; K < 1 or K > 64; NULL buffers.  pf_profile_get("delta") counts the calls of the two handle entry
 * points. */
int pf_delta(pf_handle_t* h, const float* preds, int32_t B, int32_t N, int32_t K, int64_t* pair_sum, int64_t* hist, uint8_t* nonfinite);
int pf_delta_device(pf_handle_t* h, const float* d_preds, int32_t B, int32_t N, int32_t K, int64_t* d_pair_sum, int64_t* d_hist,
                    uint8_t* d_nonfinite);
int pf_delta_host(const float* preds, int32_t B, int32_t N, int32_t K, int64_t* pair_sum, int64_t* hist, uint8_t* nonfinite);

/* ---- tree fit: how well a tree reproduces the distances it was built from (additive to ABI 5) ----
 *
 * The path-length (patristic) distances of join tables (cophenetic.phylo of R's ape) and the sums of their residuals
 * against the source's distances, bit for bit those of phyloformer_amd/fit.py::tree_fit_py.  A tree is a join table in
 * pf_nj_joins' layout, whichever of pf_nj_joins, pf_bionj_joins, pf_bme_nni and pf_bme_spr made it; its lengths are taken as
 * they are (a negative one is not clamped).  Leaves are nodes 0 .. N-1, join t makes node N + t, node 2N - 3 is the parent of
 * the last three.  T[x, y] = up(x) + up(y), each the float64 sum of the branches from the leaf up to, not beyond, the lowest
 * common node, added one after the other from +0.0.  e = (double)pred - T.  Per sequence i over j != i: ss = sum e e, fm =
 * sum (e e) / (d d) (0 where d <= 0), st = sum T, stt = sum T T, sdt = sum d T, worst = max |e| and its j (ties: the
 * smallest), summed in 64 strided accumulators that are combined pairwise at distances 32, 16, ... 1: the order is part of
 * the definition (csrc/pf_fit.hip.h, csrc/pf_fit_host.h).
 *   preds     float  [B][P_N]        pf_forward's distances, pairs i < j in lexicographic order
 *   slots     int32  [B][M][T]       M join tables per source, T = 2 (N - 3) + 3
 *   lengths   double [B][M][T]
 *   patristic double [B][M][P_N]     the tree's distances in preds' pair order; or NULL: they are kept per chunk of trees in the
 *                                    handle's workspace only (option "ws_limit_mb")
 *   rows      double [B][M][N][6]    ss, fm, st, stt, sdt, worst of every sequence
 *   worst_j   int32  [B][M][N]
 *   status    uint8  [B][M]          0 fine; 1 a NaN or an infinity in the source's distances or the tree's lengths; 2 no join
 *                                    table (a slot outside [0, N), a slot joined after it left, a == b; checked first).  A
 *                                    tree with a status has zeros everywhere and is walked by no kernel
 * pf_tree_fit takes host arrays and is synchronous; pf_tree_fit_device takes device arrays and is asynchronous on the
 * handle's stream; pf_tree_fit_host is the serial twin, without a handle or a device.  One call with B sources equals B
 * calls with one.  The node arrays of a tree (12 bytes a node) are staged in LDS up to N = 6,827 and read from global memory
 * above (option "fit_lds_bytes" lowers the switch).  Refused with PF_EINVAL before any device work, the message naming the
 * value: N < 3; N > 8,192; B < 1; M < 1; P_N >= 2^31; NULL buffers other than patristic; a tree's state above the workspace
 * limit.  pf_profile_get("tree_fit") counts the calls of the two handle entry points. */
int pf_tree_fit(pf_handle_t* h, const float* preds, const int32_t* slots, const double* lengths, int32_t B, int32_t M, int32_t N,
                double* patristic, double* rows, int32_t* worst_j, uint8_t* status);
int pf_tree_fit_device(pf_handle_t* h, const float* d_preds, const int32_t* d_slots, const double* d_lengths, int32_t B, int32_t M,
                       int32_t N, double* d_patristic, double* d_rows, int32_t* d_worst_j, uint8_t* d_status);
int pf_tree_fit_host(const float* preds, const int32_t* slots, const double* lengths, int32_t B, int32_t M, int32_t N, double* patristic,
                     double* rows, int32_t* worst_j, uint8_t* status);

/* ---- least-squares branch lengths of a fixed join table (additive to ABI 5) ----
 *
 * The ordinary-least-squares (OLS) branch lengths of join tables: the lengths that minimise the residual sum of squares
 * pf_tree_fit reports over all length vectors of the table's topology, by the closed form of Rzhetsky & Nei 1993 (FastME's
 * -w OLS), bit for bit those of phyloformer_amd/ols.py::tree_ols_py.  A tree is a join table in pf_nj_joins' layout; only its
 * slots are read.  Nodes are pf_tree_fit's; the children of join t are (the node in slot a, the node in slot b), the last node's
 * are the last three in table order.  W[v][x] is the float64 sum of leaf x's distances to the leaves of node v, added along the
 * tree (W[v] = W[a] + W[b]; r = (W[c0] + W[c1]) + W[c2]).  Per branch the sums of W over the leaves of the two subtrees below
 * it and of the sibling subtree - six sums at the most - are formed in 64 strided accumulators over the subtree's leaves in
 * the tree's leaf order and combined pairwise at distances 32, 16, ... 1; the closed form follows with every product, quotient
 * and sum rounded where ols.py writes it: the order is part of the definition (csrc/pf_ols.hip.h, csrc/pf_ols_host.h; DESIGN.md
 * section 34).
 *   preds     float  [B][P_N]        pf_forward's distances, pairs i < j in lexicographic order
 *   slots     int32  [B][M][T]       M join tables per source, T = 2 (N - 3) + 3
 *   ols       double [B][M][T]       the OLS lengths in the positions of the table's own lengths; a negative one is not clamped
 *   status    uint8  [B][M]          0 fine; 2 no join table (as pf_tree_fit; checked first); 1 a NaN or an infinity in the
 *                                    source's distances.  A tree with a status has zeros and is walked by no kernel
 * pf_tree_ols takes host arrays and is synchronous; pf_tree_ols_device takes device arrays and is asynchronous on the
 * handle's stream; pf_tree_ols_host is the serial twin, without a handle or a device.  One call with B sources equals B
 * calls with one.  The state of a tree is (2N - 2) N doubles and 7 N int32 (1.07 GB at N = 8,192): trees run side by side in
 * chunks that fit "ws_limit_mb".  Refused with PF_EINVAL before any device work, the message naming the value: N < 3;
 * N > 8,192; B < 1; M < 1; NULL buffers; a tree's state above the workspace limit.  pf_profile_get("tree_ols") counts the
 * calls of the two handle entry points. */
int pf_tree_ols(pf_handle_t* h, const float* preds, const int32_t* slots, int32_t B, int32_t M, int32_t N, double* ols, uint8_t* status);
int pf_tree_ols_device(pf_handle_t* h, const float* d_preds, const int32_t* d_slots, int32_t B, int32_t M, int32_t N, double* d_ols,
                       uint8_t* d_status);
int pf_tree_ols_host(const float* preds, const int32_t* slots, int32_t B, int32_t M, int32_t N, double* ols, uint8_t* status);

/* ---- tree rooting: MAD and midpoint roots of a join table (additive to ABI 5) ----
 *
 * Where the root of an unrooted tree is: per branch the minimal ancestor deviation (MAD; Tria, Landan & Dagan 2017) and the root
 * position that attains it, and the midpoint of the longest path, bit for bit those of phyloformer_amd/root.py::tree_root_py.  A
 * tree is a join table in pf_nj_joins' layout; no distances are read.  Nodes and the tree's leaf order are pf_tree_ols'; lengths
 * are clamped at +0.0.  D[v][x] is the path from node v to leaf x, added along the tree one column at a time; W[b][c] = 1 /
 * (D[b][c] D[b][c]), 0 where the path is 0.  Per entry k (the branch above its node v): the position lam = clamp(-S1 / (2 S0), 0,
 * L) from the sums over the pairs the branch separates, then, with t[x] = D[v][x] + lam below v and D[v][x] - lam elsewhere,
 * ssq[k] = 0.5 sum over ordered pairs of W[q][c] ((t[q] - t[c]) (t[q] - t[c])): one sequential accumulator per leaf q over all c in
 * the tree's leaf order, the leaves' sums in 64 strided accumulators combined pairwise at distances 32, 16, ... 1.  The order is
 * part of the definition (csrc/pf_root.hip.h, csrc/pf_root_host.h).
 *   slots     int32  [B][M][T]       M join tables per source, T = 2 (N - 3) + 3
 *   lengths   double [B][M][T]       their branch lengths; a negative one counts as 0
 *   ssq       double [B][M][T]       per entry the sum of squared deviations with the root on its branch; MAD = sqrt(ssq / P_N)
 *   pos       double [B][M][T]       per entry the root's distance above the branch's lower node
 *   mid       double [B][M][5]       the midpoint: entry, distance above its lower node, the pair b < c, their distance D[c][b]
 *   status    uint8  [B][M]          0 fine; 2 no join table (as pf_tree_fit; checked first); 1 a NaN or an infinity among the
 *                                    lengths.  A tree with a status has zeros and is walked by no kernel
 * pf_tree_root takes host arrays and is synchronous; pf_tree_root_device takes device arrays and is asynchronous on the
 * handle's stream; pf_tree_root_host is the serial twin, without a handle or a device.  One call with B sources equals B
 * calls with one.  The state of a tree is (2N - 2) N + N N doubles and the node arrays (1.61 GB at N = 8,192): trees run side by
 * side in chunks that fit "ws_limit_mb".  Refused with PF_EINVAL before any device work, the message naming the value: N < 3;
 * N > 8,192; B < 1; M < 1; NULL buffers; a tree's state above the workspace limit.  pf_profile_get("tree_root") counts the
 * calls of the two handle entry points. */
int pf_tree_root(pf_handle_t* h, const int32_t* slots, const double* lengths, int32_t B, int32_t M, int32_t N, double* ssq, double* pos,
                 double* mid, uint8_t* status);
int pf_tree_root_device(pf_handle_t* h, const int32_t* d_slots, const double* d_lengths, int32_t B, int32_t M, int32_t N, double* d_ssq,
                        double* d_pos, double* d_mid, uint8_t* d_status);
int pf_tree_root_host(const int32_t* slots, const double* lengths, int32_t B, int32_t M, int32_t N, double* ssq, double* pos, double* mid,
                      uint8_t* status);

/* ---- balanced minimum-evolution NNI refinement of a join table (additive to ABI 5) ----
 *
 * Balanced nearest-neighbour interchanges (BNNI, FastME's -n B) from a start tree to a local optimum of the balanced
 * tree length, with balanced branch lengths: phyloformer_amd/bme.py states the algorithm (tree, balanced averages,
 * moves, the rule delta < -1e-12 on the key (delta, c, k), lengths, the order of the output table) and DESIGN.md
 * section 21 the device form.
 *   preds        float  [B][P_N]              as pf_nj_joins
 *   start_slots  int32  [B][2 (N - 3) + 3]    the slots of a join table (pf_nj_joins' or any valid one; lengths are not
 *                                             needed): the start tree
 *   slots, lengths      [B][2 (N - 3) + 3]    the refined tree as a join table in pf_nj_joins' layout (pf_nj_format_joins_n
 *                                             writes its text): children before parents, a cluster's slot its smallest
 *                                             sequence; lengths are the balanced branch lengths
 *   steps        int32  [B]                   moves performed
 *   tree_length  double [B]                   the sum of the branch lengths = the balanced length of the tree
 *   status       uint8  [B]                   0 ok; 1 the source holds a NaN or an infinity (its results are zeros: run
 *                                             pf_bme_newick_n for such a source); 2 stopped at the cap of 16 N moves
 * pf_bme_nni takes host arrays and is synchronous.  pf_bme_nni_device takes device arrays; it synchronises the handle's
 * stream once per round of 32 steps (the host reads the flags and rebuilds the depth table of a source that came to
 * rest), so its results are complete on return too.  pf_bme_nni_host runs the same kernel bodies serially without a
 * handle or a device: slots, steps and status equal, lengths and tree_length equal bit for bit.  Sources run side by
 * side in chunks that fit "ws_limit_mb"; one source always runs whole.  Refused with PF_EINVAL before any device work:
 * N < 3, N > 16384, B < 1; NULL buffers; P_N >= 2^31; an N whose state (its table of 4N - 6 subtrees: about 56 N^2 bytes)
 * exceeds "ws_limit_mb" (the message names the bytes); a start slot outside [0, N) or a start table that is not a join
 * table.  pf_profile_get("bme_nni") counts the calls of the two handle entry points. */
int pf_bme_nni(pf_handle_t* h, const float* preds, const int32_t* start_slots, int32_t B, int32_t N, int32_t* slots, double* lengths,
               int32_t* steps, double* tree_length, uint8_t* status);
int pf_bme_nni_device(pf_handle_t* h, const float* d_preds, const int32_t* d_start_slots, int32_t B, int32_t N, int32_t* d_slots,
                      double* d_lengths, int32_t* d_steps, double* d_tree_length, uint8_t* d_status);
int pf_bme_nni_host(const float* preds, const int32_t* start_slots, int32_t B, int32_t N, int32_t* slots, double* lengths, int32_t* steps,
                    double* tree_length, uint8_t* status);

/* ---- balanced subtree pruning and regrafting of a join table (additive to ABI 5) ----
 *
 * Balanced SPR moves (FastME's -s) from a start tree to a local optimum of the balanced tree length, with balanced
 * branch lengths: phyloformer_amd/bme.py::bme_spr states the algorithm (pair table, candidates, the rule dL < -1e-12 on
 * the key (dL, S row, target edge), the chain of swaps) and DESIGN.md section 22 the device form.  Arguments, results,
 * status codes and refusals are those of the three pf_bme_nni functions above, entry point by entry point; the state of
 * one source is about 184 N^2 bytes here (the pair table of the 4N - 6 subtrees on top).  Every step forms its table from
 * scratch on the device; the handle's stream is synchronised once per round of 32 steps.  pf_bme_spr_host runs the same
 * kernel bodies serially: all results equal bit for bit.  pf_profile_get("bme_spr") counts the calls of the two handle
 * entry points.  Options: "spr_pairs_simple" (1: the pair table by the one-thread-per-entry kernel, the baseline of
 * tools/spr_bench.py; the same bits), "spr_step_cap" (> 0: moves after which a source is capped instead of 16 N). */
int pf_bme_spr(pf_handle_t* h, const float* preds, const int32_t* start_slots, int32_t B, int32_t N, int32_t* slots, double* lengths,
               int32_t* steps, double* tree_length, uint8_t* status);
int pf_bme_spr_device(pf_handle_t* h, const float* d_preds, const int32_t* d_start_slots, int32_t B, int32_t N, int32_t* d_slots,
                      double* d_lengths, int32_t* d_steps, double* d_tree_length, uint8_t* d_status);
int pf_bme_spr_host(const float* preds, const int32_t* start_slots, int32_t B, int32_t N, int32_t* slots, double* lengths, int32_t* steps,
                    double* tree_length, uint8_t* status);

/* ---- split supports of join tables: Felsenstein counts and transfer distances (additive to ABI 5) ----
 *
 * How far the R replicate trees of a source carry the splits of its reference tree; every tree is a join table in
 * pf_nj_joins' layout (pf_nj_joins', pf_bme_nni's or pf_bme_spr's), T = 2 (N - 3) + 3 slots, lengths not needed.
 * phyloformer_amd/supports.py::split_supports states the definition and DESIGN.md section 23 the device form.  Join t
 * of a table gives the split of its cluster, taken on the side without sequence 0; k_t sequences, p_t = min(k_t, N - k_t).
 * The transfer distance of reference split s (depth p) to a replicate with splits q_j is
 *   delta = min(p - 1, min_j min(h_j, N - h_j)),  h_j = popcount(s xor q_j)
 * (Lemoine et al. 2018; p - 1 is what the replicate's leaf edges give).  A replicate whose rep_flag is set contributes
 * delta = p - 1, contains no split, and its table is never read.
 *   ref_slots  int32 [B][T]        the reference tree of every source
 *   rep_slots  int32 [B][R][T]     its replicate trees
 *   rep_flag   uint8 [B][R]|NULL   != 0: the replicate has no tree (pf_nj_joins' nonfinite, status 1 of a refinement)
 *   count      int32 [B][N - 3]    replicates with delta = 0, i.e. that contain split t: Felsenstein's count
 *   transfer   int64 [B][N - 3]    the sum of delta over the replicates; the transfer bootstrap expectation is
 *                                  1 - transfer / (R (p - 1))
 *   depth      int32 [B][N - 3]    p_t
 *   status     uint8 [B]           0 ok; 1 a table of the source is no join table (its results are zeros)
 * Everything is an integer: the results do not depend on B, on the chunking or on the entry point.  pf_join_supports
 * takes host arrays, validates every table that is read as pf_bme_nni validates a start table (PF_EINVAL) and is
 * synchronous.  pf_join_supports_device takes device arrays, is asynchronous on the handle's stream and validates in
 * the kernel: a slot outside [0, N) or a join of a dead slot never indexes memory, the source gets status 1.
 * pf_join_supports_host runs the same kernel bodies serially without a handle or a device (validation as
 * pf_join_supports).  Sources run side by side in chunks that fit "ws_limit_mb"; a source whose R + 1 bitset tables
 * (about N^2 / 8 bytes each) and deltas exceed it runs in chunks of replicates.  Refused with PF_EINVAL before any
 * device work: N < 4, N > 16384, B < 1, R < 1; NULL buffers (rep_flag may be NULL); a reference table and one replicate
 * table above "ws_limit_mb" (the message names the bytes).  pf_profile_get("join_supports") counts the calls of the two
 * handle entry points. */
int pf_join_supports(pf_handle_t* h, const int32_t* ref_slots, const int32_t* rep_slots, const uint8_t* rep_flag, int32_t B, int32_t R,
                     int32_t N, int32_t* count, int64_t* transfer, int32_t* depth, uint8_t* status);
int pf_join_supports_device(pf_handle_t* h, const int32_t* d_ref_slots, const int32_t* d_rep_slots, const uint8_t* d_rep_flag, int32_t B,
                            int32_t R, int32_t N, int32_t* d_count, int64_t* d_transfer, int32_t* d_depth, uint8_t* d_status);
int pf_join_supports_host(const int32_t* ref_slots, const int32_t* rep_slots, const uint8_t* rep_flag, int32_t B, int32_t R, int32_t N,
                          int32_t* count, int64_t* transfer, int32_t* depth, uint8_t* status);

/* ---- per-taxon transfer counts: which sequences keep a branch from its support (additive to ABI 5) ----
 *
 * pf_join_supports, keeping WHICH replicate split is the closest to every reference split, and the sequences that have
 * to move for it (Lemoine et al. 2018: the per-taxon companion of the transfer bootstrap, an instability score that
 * singles out rogue taxa).  phyloformer_amd/supports.py::transfer_taxa states the definition and DESIGN.md section 27
 * the device form.  With h_j, p and delta as above, m_j = min(h_j, N - h_j), side_j = 0 if h_j <= N - h_j else 1, and j*
 * the j of the least (m_j, j).  If m_j* <= p - 1 the transfer set of (split t, replicate r) is X = s xor q_j*,
 * complemented within the N sequences if side_j* = 1, and popcount(X) = delta.  Otherwise, or if the replicate is
 * flagged, the pair is capped: nothing is attributed to any sequence.  The pair is used iff
 * 100 delta <= cutoff_percent (p - 1); a capped pair is therefore used only at cutoff_percent = 100.
 *   cutoff_percent  0 .. 100
 *   count, transfer, depth, status    exactly pf_join_supports' results
 *   moves         int64 [B][N]             the sum over t of branch_moves[t][x]
 *   used          int32 [B][N - 3]         used replicates of split t
 *   capped        int32 [B][N - 3]         used replicates that are capped
 *   branch_moves  int32 [B][N - 3][N]|NULL used, uncapped replicates with sequence x in X
 * At cutoff_percent = 100, sum_x branch_moves[t][x] + (p_t - 1) capped[t] = transfer[t].  A source with status 1 has
 * zeros everywhere.  The three forms are pf_join_supports' (host arrays and PF_EINVAL for a table that is none; device
 * arrays, asynchronous, validated in the kernel; serial without a handle), chunked as there with one more int32 per
 * (replicate, split) of state; branch_moves is the caller's array and no part of the workspace.  Refusals are
 * pf_join_supports' (the message names the bytes), and cutoff_percent outside 0 .. 100.
 * pf_profile_get("join_transfers") counts the calls of the two handle entry points. */
int pf_join_transfers(pf_handle_t* h, const int32_t* ref_slots, const int32_t* rep_slots, const uint8_t* rep_flag, int32_t B, int32_t R,
                      int32_t N, int32_t cutoff_percent, int32_t* count, int64_t* transfer, int32_t* depth, int64_t* moves, int32_t* used,
                      int32_t* capped, int32_t* branch_moves, uint8_t* status);
int pf_join_transfers_device(pf_handle_t* h, const int32_t* d_ref_slots, const int32_t* d_rep_slots, const uint8_t* d_rep_flag, int32_t B,
                             int32_t R, int32_t N, int32_t cutoff_percent, int32_t* d_count, int64_t* d_transfer, int32_t* d_depth,
                             int64_t* d_moves, int32_t* d_used, int32_t* d_capped, int32_t* d_branch_moves, uint8_t* d_status);
int pf_join_transfers_host(const int32_t* ref_slots, const int32_t* rep_slots, const uint8_t* rep_flag, int32_t B, int32_t R, int32_t N,
                           int32_t cutoff_percent, int32_t* count, int64_t* transfer, int32_t* depth, int64_t* moves, int32_t* used,
                           int32_t* capped, int32_t* branch_moves, uint8_t* status);

/* ---- majority-rule consensus of replicate join tables, with split frequencies and mean lengths (additive to ABI 5) ----
 *
 * The tree the R replicate trees of a source agree on; every tree is a join table in pf_nj_joins' layout, T = 2 (N - 3)
 * + 3 slots.  phyloformer_amd/consensus.py::join_consensus states the definition and DESIGN.md section 25 the device
 * form.  The splits of a table are those of pf_join_supports (the side without sequence 0); c(s) is the number of
 * unflagged replicates that contain s, and s is selected iff 100 c(s) > percent R, strictly.  The M <= N - 3 selected
 * splits, pairwise disjoint or nested, are ordered by (size, lowest member) ascending.
 *   rep_slots     int32  [B][R][T]       the replicate trees of every source
 *   rep_lengths   double [B][R][T]|NULL  their branch lengths (NULL: split_length and leaf_length may be NULL too)
 *   rep_flag      uint8  [B][R]|NULL     != 0: the replicate has no tree; it is never read, contains no split, counts in R
 *   percent       50 .. 99               the threshold F
 *   n_splits      int32  [B]             M
 *   count, size   int32  [B][N - 3]      c and the number of sequences of selected split i; the first M valid, zeros beyond
 *   parent        int32  [B][N - 3]      the least j > i whose split contains split i, -1: the root
 *   split_length  double [B][N - 3]      the mean, over the replicates that contain split i in ascending order, of the
 *                                        branch above its cluster there
 *   leaf_parent   int32  [B][N]          the least j whose split holds leaf x, -1: the root (always for leaf 0)
 *   leaf_length   double [B][N]          the mean of the leaf's branch over the unflagged replicates (0 where there is none)
 *   status        uint8  [B]             0 ok; 1 an unflagged table of the source is no join table; 2 the hash table or the
 *                                        selection failed (not for valid input) - every result of the source is then zero
 * The sums run in a fixed order and hold no product: the results do not depend on B, on the chunking or on the entry
 * point, bit for bit.  pf_join_consensus takes host arrays, validates every table that is read as pf_bme_nni validates a
 * start table (PF_EINVAL) and is synchronous.  pf_join_consensus_device takes device arrays, is asynchronous on the
 * handle's stream and validates in the kernel: a slot outside [0, N) or a join of a dead slot never indexes memory, the
 * source gets status 1.  pf_join_consensus_host runs the same kernel bodies serially without a handle or a device, with
 * the kernel's validation (status 1, no refusal).  Sources run side by side in chunks that fit "ws_limit_mb".  A source
 * always runs whole: its splits are counted in a hash table whose slots point into the replicates' bitset tables, which
 * therefore have to outlive the counting - chunking one source over replicates is out of scope.  Refused with PF_EINVAL
 * before any device work: N < 4, N > 16384, B < 1, R < 1, R > 65535 or R (N - 3) > 2^29; percent outside 50 .. 99; NULL
 * buffers (rep_lengths with its two outputs, and rep_flag, may be NULL); a source whose R bitset tables (about N^2 / 8
 * bytes each), hash table (12 bytes per slot, at least 2 R (N - 3) slots) and [M][R] lengths exceed "ws_limit_mb" (the
 * message names the bytes).  pf_profile_get("join_consensus") counts the calls of the two handle entry points. */
int pf_join_consensus(pf_handle_t* h, const int32_t* rep_slots, const double* rep_lengths, const uint8_t* rep_flag, int32_t B, int32_t R,
                      int32_t N, int32_t percent, int32_t* n_splits, int32_t* count, int32_t* size, int32_t* parent, double* split_length,
                      int32_t* leaf_parent, double* leaf_length, uint8_t* status);
int pf_join_consensus_device(pf_handle_t* h, const int32_t* d_rep_slots, const double* d_rep_lengths, const uint8_t* d_rep_flag, int32_t B,
                             int32_t R, int32_t N, int32_t percent, int32_t* d_n_splits, int32_t* d_count, int32_t* d_size,
                             int32_t* d_parent, double* d_split_length, int32_t* d_leaf_parent, double* d_leaf_length, uint8_t* d_status);
int pf_join_consensus_host(const int32_t* rep_slots, const double* rep_lengths, const uint8_t* rep_flag, int32_t B, int32_t R, int32_t N,
                           int32_t percent, int32_t* n_splits, int32_t* count, int32_t* size, int32_t* parent, double* split_length,
                           int32_t* leaf_parent, double* leaf_length, uint8_t* status);

/* ---- tree distances: shared splits (Robinson-Foulds), branch score and weighted RF of K join tables (additive to ABI 5) ----
 *
 * How far the K trees of a source are from each other; every tree is a join table in pf_nj_joins' layout, T = 2 (N - 3)
 * + 3 slots.  phyloformer_amd/treedist.py::join_distances_py states the definition and DESIGN.md section 35 the device
 * form.  The splits of a table are those of pf_join_supports (N - 3 per tree, the side without sequence 0); the branch
 * above join t's cluster is at the first p > 2 t + 1 with slots[p] == slots[2 t], the branch of leaf x at the first p with
 * slots[p] == x (as pf_join_consensus reads them).  For every pair i < j of unflagged trees, mirrored to (j, i):
 *   slots    int32  [B][K][T]       the trees of every source
 *   lengths  double [B][K][T]|NULL  their branch lengths (NULL: kf and wrf may be NULL too, only shared is computed)
 *   flag     uint8  [B][K]|NULL     != 0: the tree does not exist; its table is never read
 *   shared   int32  [B][K][K]       the splits both trees hold: RF = 2 (N - 3) - 2 shared, nRF = RF / (2 (N - 3))
 *   kf       double [B][K][K]       Kuhner-Felsenstein branch score: the root of the sum of d^2 over the 3 N - 6 terms d of
 *                                   treedist.py (the splits of i against j, those of j that i lacks, the N leaf branches)
 *   wrf      double [B][K][K]       weighted RF: the sum of |d| over the same terms
 *   status   uint8  [B]             0 ok; 1 an unflagged table of the source is no join table; 2 the hash table failed
 *                                   (not for valid input) - every result of the source is then zero
 * The diagonal is N - 3 and +0.0; a pair with a flagged tree, and a flagged tree's diagonal, is -1 and NaN.  The sums run
 * in a fixed order (64 strided accumulators, then halves) without contraction: the results do not depend on B, on the
 * chunking or on the entry point, bit for bit.  pf_join_distances takes host arrays, validates every table that is read
 * as pf_bme_nni validates a start table (PF_EINVAL) and is synchronous.  pf_join_distances_device takes device arrays, is
 * asynchronous on the handle's stream and validates in the kernel: a slot outside [0, N) or a join of a dead slot never
 * indexes memory, the source gets status 1.  pf_join_distances_host runs the same kernel bodies serially without a handle
 * or a device, with the kernel's validation.  Sources run side by side in chunks that fit "ws_limit_mb"; a source always
 * runs whole.  Refused with PF_EINVAL before any device work: N < 4, N > 16384, B < 1, K < 1 or K > 4096 (so K (N - 3) <
 * 2^29); NULL buffers (lengths with its two outputs, and flag, may be NULL); a source whose K bitset tables (about N^2 / 8
 * bytes each) and hash table (8 bytes per slot, at least 2 K (N - 3) slots) exceed "ws_limit_mb" (the message names the
 * bytes).  pf_profile_get("join_distances") counts the calls of the two handle entry points. */
int pf_join_distances(pf_handle_t* h, const int32_t* slots, const double* lengths, const uint8_t* flag, int32_t B, int32_t K, int32_t N,
                      int32_t* shared, double* kf, double* wrf, uint8_t* status);
int pf_join_distances_device(pf_handle_t* h, const int32_t* d_slots, const double* d_lengths, const uint8_t* d_flag, int32_t B, int32_t K,
                             int32_t N, int32_t* d_shared, double* d_kf, double* d_wrf, uint8_t* d_status);
int pf_join_distances_host(const int32_t* slots, const double* lengths, const uint8_t* flag, int32_t B, int32_t K, int32_t N,
                           int32_t* shared, double* kf, double* wrf, uint8_t* status);

/* ---- site weights: weighted forward, pattern compression, bootstrap on distinct sites (additive to ABI 5) ----
 *
 * Nothing in the network depends on a site's position, and every reduction over sites is a plain sum (the row-attention
 * statistics and the head's site mean); column attention, LayerNorm and the feed-forward act per site.  An alignment in
 * which site l occurs w_l times is therefore the alignment of its distinct sites with every sum over sites weighted by
 * w_l and L replaced by W = sum_l w_l.  Weights are floats, finite and >= 0, W > 0 per alignment;
 * a site of weight 0 is computed and counts nothing.  W is the float sum of an alignment's weights in site order, formed
 * on the device by one thread per alignment (k_weight_sums) for every entry point.
 * Bit identity: with every weight 1 the weighted calls return their unweighted twins' bits on every path; weights
 * scaled by a power of two return the same bits (short of under- / overflow).  Integer weights agree with the forward
 * of the expanded alignment to rounding - not bit for bit: the sums associate differently.
 * Path, chunking and options ("precise", "generic", "ws_limit_mb", "max_seqs", the range re-check) as for the unweighted
 * twin, chosen by the shape (N, L) of what is forwarded - never by W. */
/* idx host uint8 [B][N][L], w host float [B][L] -> out host float [B][P].  Synchronous.  Refused before any device work,
 * `out` untouched: everything pf_forward refuses; NULL weights; a negative or non-finite weight (the message names
 * alignment and position); an alignment whose weights sum to 0 (or to inf); and (PF_ESTATE) a handle whose communicator
 * has more than one rank, or option "embed_mfma". */
int pf_forward_weighted(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, const float* w, float* out);
/* The same on device buffers d_idx [B][N][L], d_w float [B][L] -> d_out [B][P]; async on the handle's stream.  The
 * weights never pass through the host: a bad weight or W == 0 is reported late, like a residue byte > 21 - the next
 * pf_synchronize / pf_memcpy_d2h on the handle returns PF_EINVAL once (results since the last one are not valid). */
int pf_forward_weighted_device(pf_handle_t* h, const uint8_t* d_idx, int32_t B, int32_t N, int32_t L, const float* d_w,
                               float* d_out);
/* pf_forward_sites with a weight per table entry: sites host int32 [S][K], w host float [S][K] -> out [B][S][P];
 * out[b][s] equals, bit for bit, pf_forward_weighted of the host-cut alignment idx[b][:, sites[s]] with weights w[s].
 * Refusals: pf_forward_sites' and pf_forward_weighted's (a bad weight is named by set and position). */
int pf_forward_sites_weighted(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, const int32_t* sites,
                              const float* w, int32_t S, int32_t K, float* out);
/* pf_bootstrap on distinct sites: out[b][r] is replicate r of pf_bootstrap's stream for `seed`, computed as
 * pf_forward_sites_weighted with the tables of pf_boot_counts - the replicate's distinct sites, ascending, weighted by
 * their multiplicities - every replicate padded with (site 0, weight 0) to K = pf_padded_sites(max_r distinct_r, L).
 * About 0.63 L sites per replicate instead of L; the tables are built on the host.  It routes by (N, K).  Equal to
 * pf_bootstrap to rounding, not bit for bit; one call with B sources equals B calls with one, bit for bit. */
int pf_bootstrap_weighted(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, int32_t R, uint64_t seed,
                          float* out);
/* Host helpers (no device, no handle; csrc/pf_weights_host.h, Python twins in phyloformer_amd/weights_sites.py).
 * pf_padded_sites: min(L, 32 * ceil(K / 32)) - a launch needs one shape and a tile is 32 tokens - or PF_EINVAL for
 * K < 1 or K > L.  Padding entries are site 0 with weight 0. */
int pf_padded_sites(int32_t K, int32_t L);
/* Replicate r (0 <= r < R) of the stream of `seed` over L sites: sites[0..K) its distinct source sites, ascending,
 * counts[0..K) their multiplicities (summing to L); both buffers hold L entries.  Returns K, or PF_EINVAL. */
int pf_boot_counts(int32_t L, int32_t R, uint64_t seed, int32_t r, int32_t* sites, int32_t* counts);
/* The distinct columns of idx host uint8 [N][L] in order of first occurrence: first[0..K) the site where each first
 * stands, count[0..K) how often it occurs; both buffers hold L entries.  Returns K, PF_EINVAL or PF_ENOMEM. */
int pf_compress_sites(const uint8_t* idx, int32_t N, int32_t L, int32_t* first, int32_t* count);
/* The classes of equal columns the default kernels' forward finds for itself (k_site_classes, option "site_dedup"): idx
 * host uint8 [B][N][L] -> srep host int32 [B][L], the smallest site whose column equals column l (l itself where the
 * column stands first), and ucount host int32 [B], the number of distinct columns.  Bytes are compared as they are (no
 * residue check).  The forward computes the column statistics of the ucount[b] first sites only and reads them for the
 * repeats - the distances keep their bits - so ucount / L tells how much of that kernel an alignment saves.  With
 * "site_dedup" 0, or L beyond the kernel's table (4096 sites), the identity.  Synchronous.  PF_EINVAL for B, N, L < 1. */
int pf_site_classes(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, int32_t* srep, int32_t* ucount);

/* ---- site-resolved distances: site map, standard errors, site profile (additive to ABI 5) ----
 *
 * The head computes one value per (pair, site), d[p][l] = softplus(w . x[p][l] + b), and a distance is their mean
 * over sites: distance[p] = mean_l d[p][l] is an exact, additive decomposition of the output over the sites of the
 * WHOLE alignment (a window of pf_forward_windows is the network's output on a CUT alignment: another question).
 * The calls below keep d from the one forward pf_forward runs anyway:
 *   map     float [B][P][L]   map[b][p][l] = d of pair p at site l
 *   se      float [B][P]      sqrt( sum_l (d[p][l] - m[p])^2 / (L (L - 1)) ), m[p] = mean_l d[p][l]; 0 for L = 1.  The
 *                             spread of the site mean: a descriptive statistic of the model's own terms, NOT a
 *                             calibrated confidence interval (sites are not independent after column attention)
 *   profile float [B][L]      mean_p d[p][l]: how much site l contributes to the distances
 * `out` equals pf_forward / pf_forward_device of the same input bit for bit, on the path that call takes for (N, L)
 * (default kernels with or without "head_fold", the float64 routes; "precise", "generic", "ws_limit_mb", "max_seqs"
 * apply unchanged).  map, se and profile are batch invariant: an alignment gets the same bits alone and anywhere in a
 * batch, whatever the chunking (a chunk's map bytes count inside "ws_limit_mb" for these calls).  The host calls are
 * synchronous and re-check ranges like pf_forward: an alignment recomputed on the float64 kernels ("recheck_above")
 * has its map / se / profile replaced together with its out; the _device calls are asynchronous on the handle's
 * stream and do not re-check.  Refused before any device work: what pf_forward refuses, NULL buffers, sizes that
 * overflow size_t, and (PF_ESTATE) a handle whose communicator has more than one rank - there is no site-sharded
 * variant, a rank would hold a slice of the map. */
/* out [B][P] as pf_forward; map [B][P][L] (host; copied one forward chunk at a time) */
int pf_forward_site_map(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, float* out, float* map);
/* device buffers; every chunk writes its slice of d_map directly */
int pf_forward_site_map_device(pf_handle_t* h, const uint8_t* d_idx, int32_t B, int32_t N, int32_t L, float* d_out,
                               float* d_map);
/* out [B][P], se [B][P], profile [B][L] (host): the moments of pf_forward_site_map's map, bit for bit; the map never
 * leaves the device and never exceeds one chunk */
int pf_forward_site_profile(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, float* out, float* se,
                            float* profile);
/* The reduction alone (csrc/pf_sitemap.hip.h), on any device map float [B][P][L] -> d_se [B][P], d_profile [B][L];
 * async on the handle's stream.  Accumulated in double, rounded to float once, no atomics: the bits are a function
 * of (P, L) and the values only.  B, P, L >= 1. */
int pf_site_moments_device(pf_handle_t* h, const float* d_map, int32_t B, int32_t P, int32_t L, float* d_se,
                           float* d_profile);

/* ---- site-sharded forward and the RCCL bootstrap ---- */
/* Site-sharded forward: this rank holds sites [l_begin, l_end) of an alignment
 * with L_total sites.  idx: host uint8 [B][N][l_end - l_begin].  Every rank
 * receives the full result in out [B][P].  The row-attention statistics are all-reduced once per
 * block and the site sums once at the end (n_blocks + 1 collectives; with B >= 2 and "overlap" = 1 the
 * batch runs as two half-batches on two streams with one communicator each: 2 (n_blocks + 1) collectives).
 * Requires pf_comm_init when the communicator has more than one rank; a partial site range
 * (l_end - l_begin < L_total) on a handle without a communicator fails with PF_ESTATE instead of
 * returning partial sums. */
int pf_forward_sharded(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N,
                       int32_t l_begin, int32_t l_end, int32_t L_total, float* out);
int pf_forward_sharded_device(pf_handle_t* h, const uint8_t* d_idx, int32_t B, int32_t N,
                              int32_t l_begin, int32_t l_end, int32_t L_total, float* d_out);
/* A rank without sites (L_total < world size: l_begin == l_end, idx may be NULL) still calls
 * pf_forward_sharded*: it joins every collective of its peers with zeros, cut into the same chunks and
 * halves.  On a handle that does not communicate an empty range is PF_EINVAL like any L < 1. */

/* RCCL bootstrap (one process per GPU).  Rank 0 calls pf_comm_unique_id and
 * ships the PF_UNIQUE_ID_BYTES bytes to the other ranks by any means
 * (torch.distributed store, file, socket); every rank then calls pf_comm_init.
 * The blob is opaque: two ncclUniqueIds, because pf_comm_init creates TWO communicators, one per
 * stream of the handle - a site-sharded forward runs its two half-batches on two streams, and a
 * communicator of its own per stream means RCCL never orders one half's all-reduce behind the
 * other's.  pf_comm_init is collective (every rank, same order) and all-or-nothing: on failure the
 * handle keeps no communicator and stays a working single-rank engine. */
#define PF_UNIQUE_ID_BYTES 256
int pf_comm_unique_id(void* id_out);
int pf_comm_init(pf_handle_t* h, const void* unique_id, int32_t rank, int32_t world_size);
int pf_comm_destroy(pf_handle_t* h);
/* Which librccl the library resolved ($PF_RCCL_LIB, else $ROCM_PATH/lib, /opt/rocm/lib, then the loader's
 * search path) and its ncclGetVersion code.  Fails with PF_ERCCL when no librccl bound to the same HIP
 * runtime as this library can be loaded. */
int pf_comm_info(char* path_out, size_t path_cap, int32_t* version);

/* ---- streams and device memory, profiling, debug taps, device properties, emulated shards, self test ---- */
/* Stream / device access for callers that time with HIP events. */
int pf_synchronize(pf_handle_t* h);
int pf_get_stream(pf_handle_t* h, void** hip_stream_out);
int pf_device_malloc(pf_handle_t* h, size_t bytes, void** out);
int pf_device_free(pf_handle_t* h, void* p);
int pf_memcpy_h2d(pf_handle_t* h, void* dst, const void* src, size_t bytes);
int pf_memcpy_d2h(pf_handle_t* h, void* dst, const void* src, size_t bytes);

/* Per-kernel HIP-event timing ("profile" = 1).  Names: "embed", "rowfin",
 * "colstats", "colfin", "main", "allreduce", "mha_qkv", "mha_attn", "mha_out", "precise", "generic",
 * "resample" (k_resample of pf_bootstrap / pf_resample_sites_device), "gather" (k_gather_sites of pf_forward_sites /
 * pf_forward_windows / pf_gather_sites_device), "site_moments" (the reduction of pf_forward_site_profile /
 * pf_site_moments_device), "gather_taxa" (k_gather_taxa of pf_forward_taxa / pf_forward_leave_one_out /
 * pf_gather_taxa_device), "loo_stats" (the reduction of pf_forward_leave_one_out / pf_loo_stats_device).
 * "weight_sums" (k_weight_sums of the weighted forwards), "place_stats" (the reduction of pf_forward_place /
 * pf_place_stats_device), "tile_combine" (k_tile_combine of pf_forward_tiled / pf_tile_combine_device), "bme_pairs" (the pair table of the first
 * step of every round of pf_bme_spr / pf_bme_spr_device: k_bme_pairs, or k_bme_pairs_simple under "spr_pairs_simple").  Totals accumulate until reset.
 * "nj_joins" returns the number of pf_nj_joins / pf_nj_joins_device calls since the last reset in *launches (counted
 * always; *total_ms = 0), "bme_nni" likewise that of pf_bme_nni / pf_bme_nni_device calls, "bme_spr" that of pf_bme_spr / pf_bme_spr_device calls.  "collectives" returns the number of all-reduces issued since the last reset in
 * *launches (counted always, no profiling option needed; *total_ms = 0); "rechecked" likewise the number of
 * alignments the range re-check (option "recheck_above") computed again on the float64 kernels. */
int pf_profile_reset(pf_handle_t* h);
int pf_profile_get(pf_handle_t* h, const char* kernel, int64_t* launches, double* total_ms);

/* Debug taps ("debug_keep" = 1), valid after a forward:
 *   "x<k>"    float [B][P][Lloc][64]  residual stream after k main kernels
 *             (x0 = embedding + pair expansion, x<k> = output of block k-1)
 *   "srow<k>" float [B][P][72]   row statistics feeding block k
 *   "ctx<k>"  float [B][Lloc][64] column context of block k
 *   "srep", "ulist" int32 [B][Lloc], "ucount" int32 [B]: the run's classes of equal columns (raw int32 bits in the
 *             float buffer; a "ulist" row is written up to ucount[b]); "plan" int32 [4 + 3 B + 1]: the routes of option
 *             "main_dedup" (csrc/pf_layout.h, main_plan_ints) - only after a forward that was routed, else PF_ESTATE
 * (the float64 path keeps only "x<k>", k >= 1, narrowed to float)
 * Returns the number of floats written (<= cap) or a negative status. */
int64_t pf_debug_read(pf_handle_t* h, const char* name, float* dst, int64_t cap);

/* Device properties the benchmark prints: name, CU count, HBM bytes. */
int pf_device_info(pf_handle_t* h, char* name_out, size_t name_cap, int32_t* cu_count,
                   uint64_t* hbm_bytes);
/* PCI address of the handle's device (hipDeviceProp_t pciDomainID / pciBusID / pciDeviceID), so that a caller
 * can find the same GPU in tools that index in PCI order (rocm_smi) whatever HIP_VISIBLE_DEVICES says. */
int pf_device_pci(pf_handle_t* h, int32_t* domain, int32_t* bus, int32_t* device);

/* Single-GPU emulation of pf_forward_sharded over `nshards` ranks (test backend): same kernels
 * and per-shard workspaces as real ranks, the RCCL all-reduces replaced by device-side sums.
 * idx: host uint8 [B][N][L]; out: host float [B][P]. */
int pf_forward_shards_emulated(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L,
                               int32_t nshards, float* out);

/* Hardware-layout self test: one wave exercises the cross-lane primitives and one
 * MFMA with known operands; `out` receives 2304 floats (layout in
 * phyloformer_amd/csrc/pf_device.hip.h::k_selftest).  tests/test_gpu_parity.py::test_hardware_layout_selftest
 * checks them against the layout the kernels assume. */
int pf_selftest(pf_handle_t* h, float* out);

/* ---- softmax multi-head attention ---------------------------------------
 *
 * The reference's MultiHeadAttention (phyloformer/attention.py:53-91: q/k/v projections :64-78,
 * QK^T / sqrt(head_dim) :81-82, softmax :83, PV :85, out_proj :89).  Nothing in the reference
 * instantiates it and no checkpoint fits it, so it is not part of pf_forward; it is provided as a
 * stand-alone operator with the module's call surface.  x, y: float [B][R][C][64]; attention runs
 * along C, independently for every (b, r) and each of the 4 heads.  Weights are nn.Linear tensors
 * ([out][in] row-major + bias).  The object shares its parent handle's device and stream and must be
 * destroyed before it.
 * Range (ABI 5): every contraction splits its operands into two fp16 limbs, so x, the weights and the
 * q / k / v projections must stay below 65504 in magnitude (any LayerNorm-ed activation does, by orders of
 * magnitude); beyond it the result is inf / NaN, not a wrong number. */
typedef struct pf_mha_weights_t {
    int32_t n_heads;     /* 4 */
    int32_t embed_dim;   /* 64 */
    const float *wq, *bq, *wk, *bk, *wv, *bv, *wo, *bo;
} pf_mha_weights_t;
typedef struct pf_mha pf_mha_t;
/* A handle with a device and a stream but no Phyloformer weights, for callers that only use the
 * stand-alone operators; pf_forward* on it fail with PF_ESTATE. */
int pf_create_bare(int device, pf_handle_t** out);
int pf_mha_create(pf_handle_t* h, const pf_mha_weights_t* w, pf_mha_t** out);
int pf_mha_destroy(pf_mha_t* m);
/* host buffers, synchronous */
int pf_mha_forward(pf_mha_t* m, const float* x, int32_t B, int32_t R, int32_t C, float* y);
/* device buffers, asynchronous on the parent handle's stream */
int pf_mha_forward_device(pf_mha_t* m, const float* d_x, int32_t B, int32_t R, int32_t C, float* d_y);

/* ---- host-side file formats of the CLI (no GPU, callable without a handle) --------------------
 *
 * pf_parse_fasta replaces load_alignment (phyloformer/data.py:11-31): `data[len]` is the whole file;
 * lines are split on '\n' and stripped of ASCII white space, a line starting with '>' opens a record
 * (id = rest of the line), other non-empty lines are residues of the current record.  Writes residue
 * indices uint8 [N][L] to `idx` (NULL = only measure) and, per record, the (offset, length) of its id
 * inside `data` to id_spans[2*N] (NULL = skip; at most max_seqs records).  Returns PF_OK and N, L, or
 *   PF_FASTA_EBYTE     byte outside the alphabet, *detail = the byte   (KeyError, data.py:26)
 *   PF_FASTA_ERAGGED   records of different lengths, *n_out still set  (ValueError from one_hot/stack)
 *   PF_FASTA_ENOHEADER residues before the first '>'                   (IndexError, data.py:26)
 *   PF_FASTA_EEMPTY    no record at all (RuntimeError from one_hot in the reference; so is N records of
 *                      length 0, which returns PF_OK with *l_out = 0)
 *   PF_FASTA_ECAP      idx_cap or max_seqs too small
 *   PF_FASTA_EUTF8     a header that bytes.decode("utf8") refuses, *detail = offset of the id in `data`
 *                      (UnicodeDecodeError at that line, data.py:22)
 * Errors are reported in file order: the first offending line decides, as in the reference's loop.
 */
#define PF_FASTA_EBYTE (-16)
#define PF_FASTA_ERAGGED (-17)
#define PF_FASTA_ENOHEADER (-18)
#define PF_FASTA_EEMPTY (-19)
#define PF_FASTA_ECAP (-20)
#define PF_FASTA_EUTF8 (-21)
int pf_parse_fasta(const char* data, int64_t len, uint8_t* idx, int64_t idx_cap, int64_t* id_spans,
                   int32_t max_seqs, int32_t* n_out, int32_t* l_out, int64_t* detail);

/* pf_format_phylip replaces vec_to_phylip (infer_alns.py:14-25): "N\n" then, per sequence,
 * "<id> d0 d1 ... dN-1\n" with "%.10f" entries of the symmetrised matrix (zero diagonal).
 * preds: float [N(N-1)/2], pairs (i<j) lexicographic; ids: N NUL-terminated strings.
 * Returns the text length in bytes (not NUL-terminated); nothing past `cap` is written, so a
 * first call with out = NULL, cap = 0 sizes the buffer. */
int64_t pf_format_phylip(const float* preds, int32_t n, const char* const* ids, char* out, int64_t cap);
/* Same with explicit id lengths (ids may then hold NUL bytes, as the reference's str ids may). */
int64_t pf_format_phylip_n(const float* preds, int32_t n, const char* const* ids, const int64_t* id_lens, char* out,
                           int64_t cap);

/* pf_nj_newick_n replaces skbio.tree.nj + the tree's text for the CLI's --trees (infer_alns.py:62-64,120-123):
 * neighbour joining (Saitou & Nei) on the symmetrised matrix of preds, float64 arithmetic, negative branch lengths
 * clamped to zero when clamp_negative != 0 (scikit-bio's default), the last three clusters joined at a trifurcation;
 * Newick text "(...);\n" with the ids as labels and Python-repr branch lengths - byte-identical to
 * phyloformer_amd/nj.py, which is pinned against FastME -m N trees of the reference's distances.  Sizing protocol as
 * pf_format_phylip (out = NULL, cap = 0 first). */
int64_t pf_nj_newick_n(const float* preds, int32_t n, const char* const* ids, const int64_t* id_lens, int32_t clamp_negative,
                       char* out, int64_t cap);

/* ---- Newick text of join tables, and of the refined and the BIONJ trees of distances (additive to ABI 5) ----
 *
 * Each of the four came with its device twin (pf_nj_joins, pf_bme_nni, pf_bme_spr, pf_bionj_joins): an ABI-5 library
 * built before that twin lacks it.  pf_nj_newick_n above came with ABI 5 itself and is always there. */
/* The Newick text of a join table (pf_nj_joins' slots / lengths [2 (n - 3) + 3] of ONE source, n >= 3): the text
 * nj.py::newick_of_joins writes for it, hence pf_nj_newick_n's when the table is that of the same distances.  No
 * device, no handle.  PF_EINVAL also for a slot outside [0, n).  Sizing protocol as pf_format_phylip. */
int64_t pf_nj_format_joins_n(const int32_t* slots, const double* lengths, int32_t n, const char* const* ids, const int64_t* id_lens,
                             int32_t clamp_negative, char* out, int64_t cap);

/* The Newick text of the neighbour-joining tree of preds refined by balanced NNIs, with balanced branch lengths (the
 * CLI's --bme; phyloformer_amd/bme.py::bme_newick_py writes the same bytes): pf_nj_newick_n's tree through
 * pf_bme_nni_host and pf_nj_format_joins_n.  n < 3 or a NaN / infinity in preds: pf_nj_newick_n's text.  No device, no
 * handle.  Sizing protocol as pf_format_phylip. */
int64_t pf_bme_newick_n(const float* preds, int32_t n, const char* const* ids, const int64_t* id_lens, int32_t clamp_negative,
                        char* out, int64_t cap);

/* The same with the tree refined by balanced SPR moves (the CLI's --spr; bme.py::spr_newick_py writes the same bytes):
 * pf_bme_spr_host in pf_bme_nni_host's place. */
int64_t pf_bme_spr_newick_n(const float* preds, int32_t n, const char* const* ids, const int64_t* id_lens, int32_t clamp_negative,
                            char* out, int64_t cap);

/* The Newick text of the BIONJ tree of preds (the CLI's --bionj; phyloformer_amd/bionj.py::bionj_newick_py writes the
 * same bytes): pf_bionj_joins_host's table through pf_nj_format_joins_n's writer.  n < 3 or a NaN / infinity in preds:
 * pf_nj_newick_n's text.  No device, no handle.  Sizing protocol as pf_format_phylip. */
int64_t pf_bionj_newick_n(const float* preds, int32_t n, const char* const* ids, const int64_t* id_lens, int32_t clamp_negative,
                          char* out, int64_t cap);

/* ---- many files per call, on native threads (ABI 4; tree_paths: ABI 5) ---------------------------
 *
 * The CLI loop (infer_alns.py:97-117) opens, parses, formats and writes one small file per alignment.
 * pf_fasta_batch_load reads and parses `count` files on up to `threads` native threads (pf_parse_fasta's
 * rules and status codes per file; PF_EIO with detail = errno when a file cannot be read) into a
 * library-owned batch object; pf_fasta_batch_infos fills per-file arrays of length count;
 * pf_fasta_batch_gather copies the residue indices of `count` (batch, file) entries, all of shape n x l,
 * into dst [count][n][l] - the input of pf_forward; pf_phylip_write_batch formats preds [count][n(n-1)/2]
 * as pf_format_phylip does, with the sequence ids the batch objects hold, and writes out_paths[k] - and, when
 * tree_paths is not NULL, the pf_nj_newick_n text of the same distances to tree_paths[k] - on up to
 * `threads` threads: status[k] = 0 or -errno.  A batch object is immutable after load: any number of threads
 * may read it; free it once, after the last use. */
typedef struct pf_fasta_batch pf_fasta_batch_t;
int pf_fasta_batch_load(const char* const* paths, int32_t count, int32_t threads, pf_fasta_batch_t** out);
void pf_fasta_batch_free(pf_fasta_batch_t* b);
int32_t pf_fasta_batch_count(const pf_fasta_batch_t* b);
int pf_fasta_batch_infos(const pf_fasta_batch_t* b, int32_t* status, int32_t* n, int32_t* l, int64_t* detail);
int pf_fasta_batch_id(const pf_fasta_batch_t* b, int32_t file, int32_t seq, const char** id, int64_t* len);
int pf_fasta_batch_gather(const pf_fasta_batch_t* const* batches, const int32_t* file_idx, int32_t count, int32_t n,
                          int32_t l, uint8_t* dst);
int pf_phylip_write_batch(const pf_fasta_batch_t* const* batches, const int32_t* file_idx, int32_t count, int32_t n,
                          const float* preds, const char* const* out_paths, const char* const* tree_paths, int32_t threads,
                          int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* PHYLOFORMER_AMD_H */
