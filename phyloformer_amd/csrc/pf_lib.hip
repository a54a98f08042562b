// libphyloformer_amd.so — host side of the C ABI declared in include/phyloformer_amd.h.
//
// Owns: the device, two streams, the prepared weights (fp32 folded copies and
// split-fp16 MFMA fragment images), two grow-only workspaces, the optional RCCL
// communicator and the launch sequence of the forward pass
// (reference: phyloformer/model.py:166-187).
//
// Launch sequence for one batch chunk (nb = n_blocks); a chunk of >= 2 alignments runs it twice, for its two
// halves, on the two streams (schedule(), driven by forward_chunk and pf_forward_shards_emulated over shard_run()'s runs):
//   launch_site_classes   k_site_classes: classes of equal alignment columns: srep, ulist, ucount (option "site_dedup"); a routed
//                         run: k_main_plan, which alignments run k_main's per-token work per distinct column ("main_dedup")
//   phase_first           k_embed: row statistics of block 0 and q' by table lookup (x0 is not written)
//   phase_block(k), k in 0..nb-1:
//       [launch_rowsum, all-reduce srow]   site-sharded runs only
//       launch_rowfin      per-tile row statistics -> row-mix matrices / fragments of every pair
//       launch_colstats    x (block 0: the embedding table), qrow, mrow -> qcol, column partials (groups or runs), both for
//                          the first site of every class only
//       launch_colfin      partials (of the site's class) -> ctx, for every site
//       launch_block_main  k_main<MID0|MID|LAST_FOLD>: row + column attention applied, FFN, next block's row statistics / head;
//                          block_kind() says which instantiation (main_kernels() is their one table, launch_main their one
//                          launch) and whether by the run's routes: launch_main_routed
//   launch_outsum         k_outsum: per-tile head sums -> distances;  [all-reduce out]: site-sharded runs only
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/phyloformer_amd.h"
#include "pf_device.hip.h"
#include "pf_mha.hip.h"
#include "pf_precise.hip.h"
#include "pf_generic.hip.h"
#include "pf_boot.hip.h"
#include "pf_sites.hip.h"
#include "pf_sitemap.hip.h"
#include "pf_sites_host.h"
#include "pf_taxa.hip.h"
#include "pf_place.hip.h"
#include "pf_tile.hip.h"
#include "pf_nj.hip.h"
#include "pf_bionj.hip.h"
#include "pf_delta.hip.h"
#include "pf_fit.hip.h"
#include "pf_ols.hip.h"
#include "pf_root.hip.h"
#include "pf_bme.hip.h"
#include "pf_support.hip.h"
#include "pf_consensus.hip.h"
#include "pf_treedist.hip.h"
#include "pf_weights.hip.h"
#include "pf_weights_host.h"
#include "pf_host_prep.h"

using namespace pfk;
using namespace pfhost;

namespace {

thread_local std::string g_create_error;

// ---- RCCL, resolved lazily so the library loads without it --------------------------------
struct PfNcclId { char internal[128]; };     // ncclUniqueId (NCCL_UNIQUE_ID_BYTES)
struct RcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, PfNcclId, int) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
// The only process-global mutable state of the library: resolved once (std::call_once), read-only afterwards.
RcclApi g_rccl;
std::string g_rccl_path;
int g_rccl_version = 0;
std::once_flag g_rccl_once;
std::string g_rccl_err;     // why the one attempt failed (empty = loaded)

// Resolution order is fixed so that the library does not depend on what else the process has mapped
// (a Python process that imported torch carries torch's own bundled librccl / HIP runtime):
// $PF_RCCL_LIB, then the ROCm installation this library was built against, then the loader's search path.
bool load_rccl_once(std::string& err) {
    std::vector<std::string> names;
    if (const char* env = std::getenv("PF_RCCL_LIB")) names.push_back(env);
    else {
        if (const char* rocm = std::getenv("ROCM_PATH")) names.push_back(std::string(rocm) + "/lib/librccl.so.1");
        names.push_back("/opt/rocm/lib/librccl.so.1");
        names.push_back("librccl.so.1");
        names.push_back("librccl.so");
    }
    void* lib = nullptr;
    std::string tried;
    for (const std::string& n : names) {
        lib = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (lib) break;
        tried += (tried.empty() ? "" : ", ") + n;
    }
    if (!lib) { err = "cannot load librccl (tried " + tried + "): " + dlerror(); return false; }
    g_rccl.GetUniqueId = reinterpret_cast<int (*)(void*)>(dlsym(lib, "ncclGetUniqueId"));
    g_rccl.CommInitRank = reinterpret_cast<int (*)(void**, int, PfNcclId, int)>(dlsym(lib, "ncclCommInitRank"));
    g_rccl.AllReduce = reinterpret_cast<int (*)(const void*, void*, size_t, int, int, void*, hipStream_t)>(
        dlsym(lib, "ncclAllReduce"));
    g_rccl.CommDestroy = reinterpret_cast<int (*)(void*)>(dlsym(lib, "ncclCommDestroy"));
    g_rccl.GetErrorString = reinterpret_cast<const char* (*)(int)>(dlsym(lib, "ncclGetErrorString"));
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.CommDestroy) {
        err = "librccl is missing required symbols";
        return false;
    }
    // RCCL and this library must sit on the same HIP runtime: two runtimes in one process own separate
    // device contexts and streams.  Compare the file that provides hipGetDeviceCount for each of them.
    Dl_info rinfo{}, hinfo{}, mine{};
    dladdr(reinterpret_cast<void*>(g_rccl.GetUniqueId), &rinfo);
    g_rccl_path = rinfo.dli_fname ? rinfo.dli_fname : "?";
    void* rccl_hip = dlsym(lib, "hipGetDeviceCount");     // resolved through librccl's own dependency chain
    if (rccl_hip && dladdr(rccl_hip, &hinfo) && dladdr(reinterpret_cast<void*>(&hipGetDeviceCount), &mine) &&
        hinfo.dli_fname && mine.dli_fname && std::strcmp(hinfo.dli_fname, mine.dli_fname) != 0) {
        err = std::string("librccl (") + g_rccl_path + ") is bound to the HIP runtime " + hinfo.dli_fname +
              " but this library uses " + mine.dli_fname + "; set PF_RCCL_LIB to the matching librccl";
        dlclose(lib);
        return false;
    }
    if (auto getv = reinterpret_cast<int (*)(int*)>(dlsym(lib, "ncclGetVersion"))) getv(&g_rccl_version);
    g_rccl.lib = lib;
    return true;
}
bool load_rccl(std::string& err) {
    std::call_once(g_rccl_once, [] { if (!load_rccl_once(g_rccl_err) && g_rccl_err.empty()) g_rccl_err = "librccl unavailable"; });
    if (g_rccl.lib) return true;
    err = g_rccl_err;
    return false;
}
constexpr int NCCL_FLOAT = 7, NCCL_DOUBLE = 8, NCCL_SUM = 0;

struct BlockDev {
    float* wimg = nullptr;     // LDS image: FRAG_END frags (as bytes) ; stored as raw
    float* consts = nullptr;   // CONST_LEN
    float* wv_lo = nullptr;    // lo fragments of THIS block's row Wv' (WVLO_FRAGS)
    float* bqk_row = nullptr;  // (host copy lives in consts of the previous stage)
    float* row_woT = nullptr;  // [64][64]
    float* row_bv = nullptr;   // [64]
    float* row_bo = nullptr;   // [64]
    float* col_bo = nullptr;   // [64] column out_proj bias (rides in the row-mix fragments, k_rowfin)
    float* col_wqk = nullptr;  // [8][64]
    float* col_bqk = nullptr;  // [8]
    float* col_wvT = nullptr;  // [64][64]
    float* col_bv = nullptr;   // [64]
};

struct ProfSlot { int kid; hipEvent_t a, b; };
const char* const KNAMES[] = {"embed", "rowfin", "colstats", "colfin", "main", "allreduce",
                              "mha_qkv", "mha_attn", "mha_out", "precise", "generic", "resample", "gather", "site_moments", "gather_taxa", "loo_stats",
                              "weight_sums", "place_stats", "tile_combine", "bme_pairs", "site_classes"};
enum { K_EMBED = 0, K_ROWFIN, K_COLSTATS, K_COLFIN, K_MAIN, K_ALLREDUCE, K_MHA_QKV, K_MHA_ATTN, K_MHA_OUT, K_PRECISE, K_GENERIC,
       K_RESAMPLE, K_GATHER, K_SITE_MOMENTS, K_GATHER_TAXA, K_LOO_STATS, K_WEIGHT_SUMS, K_PLACE_STATS, K_TILE_COMBINE, K_BME_PAIRS, K_SITE_CLASSES, K_COUNT };

// what the embed and head kernels (pfg's, for both float64 paths) read: C = 64 (precise) or Ep (generic)
struct F64Ends {
    const double* table = nullptr;                 // [22][C] relu(W + b), formed in double
    const double *hw = nullptr, *hb = nullptr;     // [C], [1]
};

// weights of the float64 path (pf_precise.hip.h), widened and transposed at pf_create
struct PreciseWeights {
    F64Ends ends;
    double* blob = nullptr;
    std::vector<pfp::AttnW> row, col;
    std::vector<pfp::FfnW> ffn;
};

// weights of the generic path (pf_generic.hip.h): padded, widened, in A-fragment order; built at pf_create for
// architectures other than (64, 4), on the first forced forward (option "generic") for (64, 4)
struct GenericWeights {
    F64Ends ends;
    bool ready = false;
    std::vector<pfg::AttnW> row, col;
    std::vector<pfg::FfnW> ffn;
};

constexpr int64_t SUB_FLOATS_DEFAULT = (int64_t)1 << 22;

// A grow-only device allocation, pointer and capacity together.  A buffer enters its owner's list
// (pf_handle::buffers, pf_mha::buffers) when it is constructed and is freed from there: a new one is one member.
struct DeviceBuffer {
    void* p = nullptr; size_t cap = 0;
    explicit DeviceBuffer(std::vector<DeviceBuffer*>& all) { all.push_back(this); }
    DeviceBuffer(const DeviceBuffer&) = delete;
    // `bytes` at least afterwards, contents not kept: no HIP call where it fits; the handle's streams drained before a
    // live allocation is replaced; empty after a failure
    int reserve(pf_handle* h, size_t bytes);
    void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
};
template <class T> struct Buffer : DeviceBuffer {
    using DeviceBuffer::DeviceBuffer;
    operator T*() const { return static_cast<T*>(p); }
};

}  // namespace

struct pf_handle {
    int device = 0;
    int n_blocks = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;  // second half-batch of an overlapped site-sharded forward
    hipStream_t cur = nullptr;      // the stream the forward's launches currently go to (stream or stream2)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipDeviceProp_t prop;
    std::string err;
    // options
    int64_t max_seqs = 200;
    bool profile = false;
    bool profile_main_only = false;  // "profile" = 2: bracket only k_main (the dominant kernel)
    bool debug_keep = false;
    int ablate = 0;
    unsigned long long* phase_prof = nullptr;  // device [8]: k_main per-phase cycle totals (experiments)
    bool phase_prof_last = false;              // phase_prof = 2: the last block's k_main launch only
    bool head_fold = true;        // option "head_fold": the last block's FFN output projection folded into the head
                                  // (k_main<MODE_LAST_FOLD>); 0 = the full FFN (k_main<MODE_LAST>, cross-check)
    bool force_rccl = false;  // tests: create a real 1-rank communicator and run the collectives
    int64_t ws_limit_bytes = (int64_t)24 << 30;  // per-chunk workspace budget
    // weights
    float* table = nullptr;       // [22][64]
    float* pair_table = nullptr;  // [484][72] block-0 row-attention contributions per residue pair (k_embed)
    bool embed_mfma = false;      // option "embed_mfma": use k_main<MODE_FIRST> instead of k_embed (cross-check)
    int colstats_fine = -1;       // option "colstats_fine": k_colstats blocks per run (1) / per group (0) / by batch (-1)
    bool colstats_ring = true;    // option "colstats_ring": x / q' of the next pairs through an LDS ring (1) or registers (0: cross-check)
    bool materialize_x0 = false;  // option "materialize_x0": k_embed writes x0 and block 0 reads it (round-1 path)
    bool site_dedup = true;       // option "site_dedup": k_colstats walks every distinct column once (0: every site, the identity map)
    int main_dedup = 1;           // option "main_dedup": k_main's per-token work once per distinct column - 1 per alignment, 0 never, 2 always
    bool stats_dedup = true;      // option "stats_dedup": the split route's row statistics once per distinct column of a pair row (k_row_stats)
    float* first_consts = nullptr;  // consts for k_main<FIRST> (only bqk used)
    float* first_img = nullptr;     // LDS image for k_main<FIRST> (only the row-statistics tail used)
    std::vector<BlockDev> blk;
    std::vector<void*> owned;     // every device allocation made at create
    std::vector<DeviceBuffer*> buffers;   // every grow-only buffer below
    // pair index tables
    int pair_n = -1;
    Buffer<int16_t> pair_i{buffers}, pair_j{buffers};
    // workspace (ws2: second half-batch of an overlapped site-sharded forward)
    Buffer<char> ws{buffers}, ws2{buffers};
    bool overlap = true;          // option "overlap": two half-batches on two streams when collectives run
    int reserve_cus = 8;          // option "reserve_cus": CUs the persistent kernels leave to RCCL then
    Buffer<uint8_t> d_idx{buffers};
    Buffer<float> d_out{buffers};
    Buffer<uint8_t> d_rep{buffers};       // forward_derived: one chunk of derived alignments (grow-only)
    Buffer<int32_t> d_map{buffers};       // pf_forward_sites / pf_forward_windows: the site map (grow-only)
    // pf_forward_site_map / pf_forward_site_profile (grow-only): one chunk's map of head terms, the partial column sums
    // of its reduction, and the reduced se [B][P] / profile [B][L] of a host call
    Buffer<float> d_smap{buffers}, d_se{buffers}, d_prof{buffers};
    Buffer<double> d_mpart{buffers};
    // the taxon-axis analyses (TaxonCuts: leave-one-out, placement, tiling): what one sub-call's reduction reads beside
    // h->d_out and what it writes, carved from one grow-only buffer - the three are never live together
    Buffer<char> d_sub{buffers};
    int64_t sub_floats = SUB_FLOATS_DEFAULT;    // option "sub_floats": distances one sub-call may hold on the device
    // pf_forward_tiled / pf_tile_combine_device: the plan of the last (N, M) and its two device tables
    // (pftile::table_arrays), carved from one grow-only buffer
    pftile::Plan tiled_plan;
    pftile::Tables tiled_tab;
    Buffer<char> d_tiled_tab{buffers};
    // pf_nj_joins / pf_nj_joins_device (grow-only): the state of one chunk of sources (d, r, partial minima, active
    // slots), and the staging of a host call's chunk (lengths, preds, slots, flags).  pf_bionj_joins / _device use both
    // for their own state (pf_bionj_host.h: state_arrays) and the same staging: calls follow each other on the stream.
    Buffer<char> d_nj{buffers}, d_nj_io{buffers};
    int64_t nj_calls = 0;        // calls since the last pf_profile_reset ("nj_joins")
    int64_t bionj_calls = 0;     // likewise pf_bionj_joins / pf_bionj_joins_device ("bionj_joins")
    // pf_delta (grow-only): the staging of the host entry point's distances and results; the kernels keep no state
    Buffer<char> d_delta_io{buffers};
    int64_t delta_calls = 0;     // pf_delta / pf_delta_device calls since the last pf_profile_reset ("delta")
    bool delta_atomic = true;    // option "delta_atomic": 0 = k_delta_pairs (the comparison of tools/delta_bench.py)
    // pf_tree_fit / pf_tree_fit_device (grow-only): the node arrays (and, without the caller's patristic, the tree's
    // distances) of one chunk of trees, and the staging of the host entry point's arrays
    Buffer<char> d_fit{buffers}, d_fit_io{buffers};
    int64_t fit_calls = 0;       // pf_tree_fit / pf_tree_fit_device calls since the last pf_profile_reset ("tree_fit")
    int64_t fit_lds_bytes = pffit::LDS_MAX_BYTES;   // option "fit_lds_bytes": what k_fit_pairs may stage in LDS; tests
    // pf_tree_ols / pf_tree_ols_device (grow-only): the column sums and the node arrays of one chunk of trees, and the
    // staging of the host entry point's arrays
    Buffer<char> d_ols{buffers}, d_ols_io{buffers};
    int64_t ols_calls = 0;       // pf_tree_ols / pf_tree_ols_device calls since the last pf_profile_reset ("tree_ols")
    // pf_tree_root / pf_tree_root_device (grow-only): the path lengths, the weights and the node arrays of one chunk of trees,
    // and the staging of the host entry point's arrays
    Buffer<char> d_root{buffers}, d_root_io{buffers};
    int64_t root_calls = 0;      // pf_tree_root / pf_tree_root_device calls since the last pf_profile_reset ("tree_root")
    // pf_bme_nni / pf_bme_nni_device (grow-only): the state of one chunk of sources (pf_bme.hip.h: carve) and the
    // staging of the host entry point's distances
    Buffer<char> d_bme{buffers};
    Buffer<float> d_bme_preds{buffers};
    int64_t bme_calls = 0;       // calls since the last pf_profile_reset ("bme_nni")
    int64_t spr_calls = 0;       // likewise pf_bme_spr / pf_bme_spr_device ("bme_spr")
    bool spr_pairs_simple = false;   // option "spr_pairs_simple": T by k_bme_pairs_simple (the baseline of tools/spr_bench.py)
    int64_t spr_step_cap = 0;    // option "spr_step_cap": moves after which pf_bme_spr caps a source (0: 16 N)
    // pf_join_supports / pf_join_supports_device (grow-only): the state of one chunk (pf_support.hip.h: carve), the
    // whole call's tree flags, and the staging of the host entry point's tables and results
    Buffer<char> d_sup{buffers}, d_sup_io{buffers};
    Buffer<uint8_t> d_sup_bad{buffers};
    int64_t sup_calls = 0;       // calls since the last pf_profile_reset ("join_supports")
    int64_t transfer_calls = 0;  // ("join_transfers": pf_join_transfers / pf_join_transfers_device)
    // pf_join_consensus / pf_join_consensus_device (grow-only): the state of one chunk of sources (pf_consensus.hip.h:
    // carve) and the staging of the host entry point's tables, lengths and results
    Buffer<char> d_con{buffers}, d_con_io{buffers};
    int64_t con_calls = 0;       // calls since the last pf_profile_reset ("join_consensus")
    // pf_join_distances / pf_join_distances_device (grow-only): the state of one chunk of sources (pf_treedist.hip.h:
    // carve) and the staging of the host entry point's tables, lengths and results
    Buffer<char> d_td{buffers}, d_td_io{buffers};
    int64_t td_calls = 0;        // calls since the last pf_profile_reset ("join_distances")
    // weighted forwards (grow-only): the weight rows of a host call or of one chunk of derived alignments, what
    // k_weight_sums made of a call's rows ([..][4], pf_weights.hip.h), and the weight table of pf_forward_sites_weighted
    Buffer<float> d_w{buffers}, d_wst{buffers}, d_wtab{buffers};
    // comm: one RCCL communicator per stream (comm[1] serves stream2), created together by pf_comm_init, so that
    // RCCL never has to order one half-batch's collectives behind the other's with an implicit cross-stream wait
    void* comm[2] = {nullptr, nullptr};
    int rank = 0, world = 1;
    int64_t coll_calls = 0;      // collectives issued since the last pf_profile_reset ("collectives")
    bool sharded_call = false;   // set by pf_forward_sharded* for the duration of the call
    bool reducing = false;       // this forward issues collectives (persistent kernels leave reserve_cus CUs free)
    bool two_streams = true;     // option "two_streams": forwards of >= 2 alignments run as two free-running half-batches
                                 // on two streams, each filling the other's kernel tails and small kernels (+2.5 %
                                 // at 60 x 500 batch 16, +4.7 % at 60 x 2000 batch 4; same bits: tools/two_streams_compare.py)
    // profiling
    std::vector<ProfSlot> pending;
    std::vector<hipEvent_t> free_events;
    int64_t prof_n[K_COUNT] = {0};
    double prof_ms[K_COUNT] = {0};
    // debug taps
    std::map<std::string, std::vector<float>> taps;
    // A/B runs: PF_ROW_TILES / PF_FLAT_TILES, read once at creation (-1 = choose from the shape)
    int tile_force = -1;
    // float64 path for ill-conditioned shapes (pf_precise.hip.h): option "precise" -1 = by shape, 0 = never, 1 = always
    int precise = -1;
    // Range re-check of the host entry points (forward_host_impl): an alignment whose largest predicted distance exceeds
    // recheck_above substitutions per site is computed again on the float64 kernels (option "recheck_above", 0 = off;
    // only when "precise" is -1).  An ABSOLUTE bound of 1e-4 on a value of 10 asks for 1e-5 relative - fp32's own level,
    // where the default kernels sit (<= 8.7e-6 of the largest distance in 21,600 soak cases) and where the fp32
    // reference itself is 5e-5 from its float64 evaluation; no alignment gets there (the reference's test data and
    // BASELINE's configurations end at 5.0), uniformly random residues do (9-13).
    double recheck_above = 8.0;
    int64_t rechecked = 0;       // alignments recomputed since the last pf_profile_reset ("rechecked")
    // fp16 operand ranges of the default kernels, from the checkpoint (check_f16_ranges): false = this checkpoint's
    // weights could overflow an fp16 MFMA operand, every forward takes the float64 kernels; f16_vmax_col = bound of the
    // column attention's |v| (the column-apply operand is <= P * f16_vmax_col / 16)
    bool f16_ok = true;
    double f16_vmax_col = 0.0;
    double f16_bounds[5] = {0, 0, 0, 0, 0};   // hidden, row-mix base * 64, weights, out_proj biases, out_proj row sums ("f16_ranges" debug read)
    char f16_why[320] = {0};
    bool precise_ffn_valu = false;   // option "precise_ffn_valu": the float64 FFN on the VALU instead of the matrix cores (cross-check)
    PreciseWeights pw;
    Buffer<char> wsp{buffers};     // workspace of the float64 paths (precise and generic)
    // generic path (pf_generic.hip.h): arch_generic = the architecture is not (64, 4), every forward runs there;
    // option "generic" = 1 sends a (64, 4) handle's forwards there too (its image is built from blob_copy then)
    bool arch_generic = false;
    int generic = 0;
    pfg::Arch garch{};
    GenericWeights gw;
    std::vector<float> blob_copy;
    // sticky "residue byte > 21 seen" flag: pinned host memory the kernels write through its device alias
    // ([1]: "site map entry out of range seen", k_gather_sites of pf_gather_sites_device; [2]: "bad site weight seen",
    // k_weight_sums of pf_forward_weighted_device)
    unsigned* bad_idx_host = nullptr;
    unsigned* bad_idx_dev = nullptr;
};

namespace {

int fail(pf_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return code;
}

#define HIPCHK(h, call)                                                                 \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail((h), e_ == hipErrorOutOfMemory ? PF_ENOMEM : PF_EHIP, "%s: %s", \
                        #call, hipGetErrorString(e_));                                  \
    } while (0)

template <typename T>
int upload(pf_handle* h, const std::vector<T>& v, float** out) {
    void* p = nullptr;
    HIPCHK(h, hipMalloc(&p, v.size() * sizeof(T)));
    h->owned.push_back(p);
    HIPCHK(h, hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = reinterpret_cast<float*>(p);
    return PF_OK;
}

int DeviceBuffer::reserve(pf_handle* h, size_t bytes) {
    if (p && bytes <= cap) return PF_OK;
    hipError_t e = hipSuccess;
    if (p) {
        e = hipStreamSynchronize(h->stream);
        if (e == hipSuccess && h->stream2) e = hipStreamSynchronize(h->stream2);
        release();
    }
    if (e == hipSuccess && (e = hipMalloc(&p, bytes ? bytes : 1)) != hipSuccess) p = nullptr;
    if (e != hipSuccess)
        return fail(h, e == hipErrorOutOfMemory ? PF_ENOMEM : PF_EHIP, "device buffer of %zu bytes: %s", bytes, hipGetErrorString(e));
    cap = bytes;
    return PF_OK;
}

// fp16 operand ranges (pf_device.hip.h): the split MFMA operands must stay below 65504.  LayerNorm output is bounded
// by construction (|x~| <= sqrt(63), ||x~||_2 <= 8); everything else by the checkpoint's weights:
//   hidden   2 a |W1' x~ + b1'| <= 2 (||W1' a row||_2 * 8 + |b1' a|)           (gelu_scaled returns at most 2 |x|)
//   M_base   sum_d |Wo[c][16h+d]| * (||Wv' row||_2 * 8 + |bv'|), times <= 64    (k_rowfin's a_scale, L_total <= 2^20)
//   column   q' / mean(q') * |v| / 16 <= P * vmax_col / 16                       (checked per shape, f16_range_ok)
// The five shipped checkpoints sit at 61 / 196 / 30 (P = 19,900 gives 37,600).  A checkpoint outside the range is not
// refused: its forwards run on the float64 kernels (use_precise).
//   biases   |row bo|, |col bo|: k_rowfin splits both out_proj biases into K slots 4 and 5 of the row-mix fragments
// A NaN passes every std::max and every "<" below, so the blob is also tested entry by entry (finite).
//
// The low side.  Below 2^-3 the lo limb is subnormal: the pair carries such a value to an ABSOLUTE 2^-25, whatever its
// size, and the partner operand multiplies that error.  A checkpoint that holds the same function with v small and
// out_proj large (or W1 large and W2 small) loses what the shipped balance keeps; measured on MI355X with exact
// power-of-two rescalings of pf, the error grows in proportion to the partner's bound:
//   wo_l1    max_c sum_hd |Wo[c][hd]|, row and column out_proj: multiplies the error of v (row: Wv' x~; column:
//            q' ctx / 16).  Shipped <= 27; at 64 x that the column attention leaves the per-buffer caps (distances
//            6.3e-5 off), at 4,096 x the row attention's distances are 2.4e-4 off.
//   vmax_col multiplies the error of a small column out_proj: 1.6e-10 x vmax_col of x's largest entry.  Shipped 30.
//   hidden   multiplies the error of a small W2: 8.8e-10 x hidden of x's largest entry.  Shipped 61.
// Limits (F16_LO_*): where the added error stays near 3e-6 of a buffer, a third of what the six blocks may add up to
// under the 1e-4 caps.  The same verdict as above: outside, the float64 kernels run.
struct F16Ranges { double hidden = 0, mbase = 0, vmax_col = 0, wmax = 0, bias = 0, wo_l1 = 0; bool finite = true; };
void f16_note_attn(const std::vector<float>& wv, const std::vector<float>& bv, const float* wo, bool col, F16Ranges* r) {
    double vmax[E];
    for (int hd = 0; hd < E; ++hd) {
        double n2 = 0;
        for (int c = 0; c < E; ++c) { n2 += (double)wv[(size_t)hd * E + c] * wv[(size_t)hd * E + c]; r->wmax = std::max(r->wmax, std::fabs((double)wv[(size_t)hd * E + c])); }
        vmax[hd] = std::sqrt(n2) * 8.0 + std::fabs((double)bv[hd]);
        if (col) r->vmax_col = std::max(r->vmax_col, vmax[hd]);
    }
    for (int c = 0; c < E; ++c)
        for (int hh = 0; hh < NH; ++hh) {
            double m = 0;
            for (int d = 0; d < HD; ++d) { m += std::fabs((double)wo[(size_t)c * E + 16 * hh + d]) * vmax[16 * hh + d]; r->wmax = std::max(r->wmax, std::fabs((double)wo[(size_t)c * E + 16 * hh + d]) * (col ? COLAPPLY_A_SCALE : 1.0)); }
            if (!col) r->mbase = std::max(r->mbase, m);
        }
    for (int c = 0; c < E; ++c) {
        double l1 = 0;
        for (int hd = 0; hd < E; ++hd) l1 += std::fabs((double)wo[(size_t)c * E + hd]);
        r->wo_l1 = std::max(r->wo_l1, l1);
    }
}
void f16_note_ffn(const std::vector<float>& w1a, const std::vector<float>& b1a, const std::vector<float>& w2s, F16Ranges* r) {
    for (int j = 0; j < FF; ++j) {
        double n2 = 0;
        for (int c = 0; c < E; ++c) { n2 += (double)w1a[(size_t)j * E + c] * w1a[(size_t)j * E + c]; r->wmax = std::max(r->wmax, std::fabs((double)w1a[(size_t)j * E + c])); }
        r->hidden = std::max(r->hidden, 2.0 * (std::sqrt(n2) * 8.0 + std::fabs((double)b1a[j])));
    }
    for (float v : w2s) r->wmax = std::max(r->wmax, std::fabs((double)v));
}
constexpr double F16_LIMIT = 60000.0;            // (65504 with a margin for the rounding of the bounds themselves)
constexpr double F16_LO_HIDDEN = 8192.0, F16_LO_VMAX_COL = 16384.0, F16_LO_WO_L1 = 512.0;    // the low side, above
void check_f16_ranges(pf_handle* h, const F16Ranges& r) {
    h->f16_vmax_col = r.vmax_col;
    h->f16_bounds[0] = r.hidden; h->f16_bounds[1] = r.mbase * 64.0; h->f16_bounds[2] = r.wmax; h->f16_bounds[3] = r.bias;
    h->f16_bounds[4] = r.wo_l1;
    const bool finite = r.finite && std::isfinite(r.hidden) && std::isfinite(r.mbase) && std::isfinite(r.vmax_col) &&
                        std::isfinite(r.wmax) && std::isfinite(r.bias) && std::isfinite(r.wo_l1);
    const bool range = r.hidden < F16_LIMIT && r.mbase * 64.0 < F16_LIMIT && r.wmax < F16_LIMIT && r.bias < F16_LIMIT;
    const bool low = r.hidden < F16_LO_HIDDEN && r.vmax_col < F16_LO_VMAX_COL && r.wo_l1 < F16_LO_WO_L1;
    h->f16_ok = !PF_F16 || (finite && range && low);
    if (!h->f16_ok)
        snprintf(h->f16_why, sizeof h->f16_why, "fp16 operands: hidden %.3g (limit %.0f), row-mix base %.3g, weights %.3g, out_proj biases %.3g "
                 "(limit %.0f), column |v| %.3g (limit %.0f), out_proj row sums %.3g (limit %.0f)%s", r.hidden, F16_LO_HIDDEN, r.mbase * 64.0,
                 r.wmax, r.bias, F16_LIMIT, r.vmax_col, F16_LO_VMAX_COL, r.wo_l1, F16_LO_WO_L1, r.finite ? "" : "; non-finite entries");
}
// per forward: the column-apply operand q' / mean(q') * v / 16 <= P * vmax_col / 16, and q' / mean(q') <= L_total on
// the row side is covered up to 2^20 sites by k_rowfin's b_scale
bool f16_range_ok(const pf_handle* h, int N, int L_total) {
    if (!PF_F16) return true;
    const double P = (double)N * (N - 1) / 2;
    return h->f16_ok && P * h->f16_vmax_col * COLAPPLY_B_SCALE < F16_LIMIT && L_total <= (1 << 20);
}

// the default kernels' operands from a (64, 4) checkpoint; blob_len: the floats the caller's blob really holds
int prepare_weights(pf_handle* h, const BlobView& view, uint64_t blob_len) {
    if ((uint64_t)view.len != blob_len)
        return fail(h, PF_EINVAL, "weight blob has %llu floats, expected %llu",
                    (unsigned long long)blob_len, (unsigned long long)view.len);
    std::vector<float> table((size_t)NA * E);
    build_embed_table(view, E, E, table.data());
    int rc = upload(h, table, &h->table);
    if (rc) return rc;

    const int nb = (int)view.ffn.size();
    h->blk.resize(nb);

    {
        std::vector<float> ptab;
        build_pair_table(table.data(), view.row[0], ptab);
        if ((rc = upload(h, ptab, &h->pair_table))) return rc;
    }
    F16Ranges ranges;
    for (size_t i = 0; i < view.len; ++i) ranges.finite = ranges.finite && std::isfinite(view.emb_w[i]);   // (the blob starts at emb_w)
    std::vector<std::vector<float>> row_bqk(nb);
    std::vector<std::vector<uint16_t>> row_tail(nb);
    for (int k = 0; k < nb; ++k) {
        BlockDev& d = h->blk[k];
        const AttnHost& r = view.row[k];
        const AttnHost& c = view.col[k];
        // ---- row attention of block k
        std::vector<float> wq, bq, wk, bk, wv, bv;
        fold(r.wq, r.bq, r.g, r.b, NH, E, wq, bq);
        fold(r.wk, r.bk, r.g, r.b, NH, E, wk, bk);
        fold(r.wv, r.bv, r.g, r.b, E, E, wv, bv);
        f16_note_attn(wv, bv, r.wo, false, &ranges);
        for (int cc = 0; cc < E; ++cc) ranges.bias = std::max({ranges.bias, std::fabs((double)r.bo[cc]), std::fabs((double)c.bo[cc])});
        for (float v : wq) ranges.wmax = std::max(ranges.wmax, std::fabs((double)v));
        for (float v : wk) ranges.wmax = std::max(ranges.wmax, std::fabs((double)v));
        row_tail[k].assign((size_t)(FRAG_END - FRAG_WV) * 8, 0);
        std::vector<uint16_t> wvlo((size_t)WVLO_FRAGS * 8);
        pack_row_stats(wv.data(), wq.data(), wk.data(), row_tail[k].data(), wvlo.data());
        std::copy(wvlo.begin(), wvlo.begin() + (size_t)WVLO_LDS * 64 * 8, row_tail[k].begin() + (size_t)(FRAG_WVLO - FRAG_WV) * 8);
        if ((rc = upload(h, wvlo, &d.wv_lo))) return rc;
        row_bqk[k].assign(8, 0.f);
        for (int i = 0; i < 4; ++i) { row_bqk[k][i] = bq[i]; row_bqk[k][4 + i] = bk[i]; }
        std::vector<float> woT((size_t)E * E);
        for (int cc = 0; cc < E; ++cc)
            for (int hd = 0; hd < E; ++hd) woT[(size_t)hd * E + cc] = r.wo[(size_t)cc * E + hd];
        if ((rc = upload(h, woT, &d.row_woT))) return rc;
        if ((rc = upload(h, bv, &d.row_bv))) return rc;
        if ((rc = upload(h, std::vector<float>(r.bo, r.bo + E), &d.row_bo))) return rc;
        if ((rc = upload(h, std::vector<float>(c.bo, c.bo + E), &d.col_bo))) return rc;
        // ---- column attention of block k
        std::vector<float> cwq, cbq, cwk, cbk, cwv, cbv;
        fold(c.wq, c.bq, c.g, c.b, NH, E, cwq, cbq);
        fold(c.wk, c.bk, c.g, c.b, NH, E, cwk, cbk);
        fold(c.wv, c.bv, c.g, c.b, E, E, cwv, cbv);
        f16_note_attn(cwv, cbv, c.wo, true, &ranges);
        std::vector<float> wqk((size_t)8 * E), bqk(8);
        std::copy(cwq.begin(), cwq.end(), wqk.begin());
        std::copy(cwk.begin(), cwk.end(), wqk.begin() + 4 * E);
        for (int i = 0; i < 4; ++i) { bqk[i] = cbq[i]; bqk[4 + i] = cbk[i]; }
        if ((rc = upload(h, wqk, &d.col_wqk))) return rc;
        if ((rc = upload(h, bqk, &d.col_bqk))) return rc;
        std::vector<float> wvT((size_t)E * E);
        for (int hd = 0; hd < E; ++hd)
            for (int cc = 0; cc < E; ++cc) wvT[(size_t)cc * E + hd] = cwv[(size_t)hd * E + cc];
        if ((rc = upload(h, wvT, &d.col_wvT))) return rc;
        if ((rc = upload(h, cbv, &d.col_bv))) return rc;
    }
    for (int k = 0; k < nb; ++k) {
        BlockDev& d = h->blk[k];
        // ---- LDS image of k_main(k): FFN + column out_proj
        const FfnHost& f = view.ffn[k];
        std::vector<float> w1f, b1f;
        fold(f.w1, f.b1, f.g, f.b, FF, E, w1f, b1f);
        // hidden pre-activations are carried as a*h, a = sqrt(log2(e)/2) (see gelu_split_pair);
        // W2 absorbs 1/a
        const double alpha = std::sqrt(0.5 * 1.4426950408889634074);
        for (auto& v : w1f) v = (float)((double)v * alpha);
        for (auto& v : b1f) v = (float)((double)v * alpha);
        std::vector<float> w2s((size_t)E * FF);
        for (size_t i = 0; i < w2s.size(); ++i) w2s[i] = (float)((double)f.w2[i] / alpha * 0.5);   // gelu_scaled returns 2*a*gelu
        f16_note_ffn(w1f, b1f, w2s, &ranges);
        std::vector<uint16_t> img((size_t)FRAG_END * 8);
        pack_frags(w1f.data(), FF, E, FF, img.data() + (size_t)FRAG_W1 * 8);
        pack_frags(w2s.data(), E, FF, E, img.data() + (size_t)FRAG_W2 * 8);
        pack_frags(view.col[k].wo, E, E, E, img.data() + (size_t)FRAG_WO * 8, COLAPPLY_A_SCALE);   // B side carries the inverse
        if (k + 1 < nb) std::copy(row_tail[k + 1].begin(), row_tail[k + 1].end(), img.begin() + (size_t)FRAG_WV * 8);
        float c0 = 0.f;
        if (k + 1 == nb) {
            // the last block's tail (no next row attention) carries the folded head: u = W2^T head_w, c0
            float u[FF];
            fold_head(f.w2, f.b2, view.head_w, view.head_b[0], 1.0 / alpha * 0.5, u, &c0);
            std::memcpy(img.data() + (size_t)FRAG_U * 8, u, sizeof(u));
        }
        if ((rc = upload(h, img, &d.wimg))) return rc;
        std::vector<float> cst(CONST_LEN, 0.f);
        std::copy(b1f.begin(), b1f.end(), cst.begin() + CONST_B1);
        std::copy(f.b2, f.b2 + E, cst.begin() + CONST_B2);
        if (k + 1 < nb) std::copy(row_bqk[k + 1].begin(), row_bqk[k + 1].end(), cst.begin() + CONST_BQK);
        std::copy(view.head_w, view.head_w + E, cst.begin() + CONST_HW);
        cst[CONST_HB] = view.head_b[0];
        cst[CONST_C0] = c0;
        std::copy(view.col[k].bo, view.col[k].bo + E, cst.begin() + CONST_BOC);
        if ((rc = upload(h, cst, &d.consts))) return rc;
    }
    std::vector<float> cst0(CONST_LEN, 0.f);
    std::copy(row_bqk[0].begin(), row_bqk[0].end(), cst0.begin() + CONST_BQK);
    std::vector<uint16_t> img0((size_t)FRAG_END * 8, 0);
    std::copy(row_tail[0].begin(), row_tail[0].end(), img0.begin() + (size_t)FRAG_WV * 8);
    check_f16_ranges(h, ranges);
    if ((rc = upload(h, img0, &h->first_img))) return rc;
    return upload(h, cst0, &h->first_consts);
}

int ensure_pairs(pf_handle* h, int N) {
    if (h->pair_n == N) return PF_OK;
    const int P = N * (N - 1) / 2;
    std::vector<int16_t> pi(P), pj(P);
    int k = 0;
    for (int i = 0; i < N; ++i)  // model.py:13-17
        for (int j = i + 1; j < N; ++j) { pi[k] = (int16_t)i; pj[k] = (int16_t)j; ++k; }
    h->pair_n = -1;                      // (a failure below leaves no table that passes for N's)
    int rc = h->pair_i.reserve(h, P * sizeof(int16_t));
    if (rc || (rc = h->pair_j.reserve(h, P * sizeof(int16_t)))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->pair_i, pi.data(), P * sizeof(int16_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->pair_j, pj.data(), P * sizeof(int16_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->pair_n = N;
    return PF_OK;
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

TilePlan tile_plan(const pf_handle* h, int P, int Lloc) { return tile_plan_core(P, Lloc, h->tile_force); }

// The default kernels' workspace as its list (pf_host_prep.h) under the handle's options; it leaves k_colstats' plan in w too.
static_assert(WS_CPART == CPART, "the workspace list sizes k_colstats' partials");
auto workspace_list(const pf_handle* h, Workspace& w, int B, int P, int Lloc) {
    return [=, &w](auto& v) { workspace_arrays(v, w, B, P, Lloc, h->colstats_fine, h->tile_force); };
}

int ensure_workspace(pf_handle* h, int B, int P, int Lloc, Workspace* w, bool second = false) {
    auto list = workspace_list(h, *w, B, P, Lloc);
    Buffer<char>& ws = second ? h->ws2 : h->ws;
    if (const int rc = ws.reserve(h, pfspan::measure(list, 256))) return rc;
    pfspan::carve(ws, list, 256);
    return PF_OK;
}

hipEvent_t get_event(pf_handle* h) {
    if (!h->free_events.empty()) { hipEvent_t e = h->free_events.back(); h->free_events.pop_back(); return e; }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
}
struct ProfScope {
    pf_handle* h; int kid; hipEvent_t a{}, b{};
    bool on;
    ProfScope(pf_handle* h_, int kid_, bool timed = true) : h(h_), kid(kid_) {
        on = timed && h->profile && (!h->profile_main_only || kid_ == K_MAIN);
        if (on) { a = get_event(h); b = get_event(h); hipEventRecord(a, h->cur); }
    }
    ~ProfScope() {
        if (on) { hipEventRecord(b, h->cur); h->pending.push_back({kid, a, b}); }
    }
};
void drain_profile(pf_handle* h) {
    if (h->pending.empty()) return;
    hipStreamSynchronize(h->stream);
    if (h->stream2) hipStreamSynchronize(h->stream2);
    for (auto& s : h->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) { h->prof_n[s.kid]++; h->prof_ms[s.kid] += ms; }
        h->free_events.push_back(s.a);
        h->free_events.push_back(s.b);
    }
    h->pending.clear();
}

int save_tap(pf_handle* h, const std::string& name, const float* dptr, size_t n) {
    std::vector<float>& v = h->taps[name];
    v.resize(n);
    HIPCHK(h, hipStreamSynchronize(h->cur));
    HIPCHK(h, hipMemcpy(v.data(), dptr, n * sizeof(float), hipMemcpyDeviceToHost));
    return PF_OK;
}

// Collectives belong to the site-sharded entry points only: pf_forward / pf_forward_device on a handle
// that carries a communicator (alignment-level data parallelism) must not reduce across ranks.
int allreduce(pf_handle* h, void* buf, size_t count, int dtype = NCCL_FLOAT) {
    if (!h->sharded_call) return PF_OK;
    if (h->world <= 1 && !h->comm[0]) return PF_OK;
    if (!h->comm[0]) return fail(h, PF_ESTATE, "sharded forward on %d ranks needs pf_comm_init", h->world);
    ProfScope ps(h, K_ALLREDUCE);
    void* comm = h->comm[(h->cur == h->stream2 && h->stream2) ? 1 : 0];    // the stream's own communicator
    ++h->coll_calls;
    int rc = g_rccl.AllReduce(buf, buf, count, dtype, NCCL_SUM, comm, h->cur);
    if (rc != 0)
        return fail(h, PF_ERCCL, "ncclAllReduce failed: %s",
                    g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "?");
    return PF_OK;
}

// ---- k_main's launches ----------------------------------------------------------------------------
// What a launch instantiates k_main with: the mode, whether it writes the head's site map or reads site weights, the
// route; the tiling (FLAT) is the run's.  HEAD_PARTS: k_head_parts, no mode of k_main but a kernel on its arguments.
enum { PLAIN = 0, SITEMAP = 1, WEIGHTED = 2 };
constexpr int HEAD_PARTS = MODE_STATS + 1;
struct MainKind { int mode, flavour = PLAIN, route = ROUTE_ALL; };
using MainKernel = void (*)(MainArgs);
struct MainRow { MainKind kind; bool flat; MainKernel fn; };
const std::vector<MainRow>& main_kernels();      // (the table stands behind the launches that name k_embed and k_colstats)

// The kernel of (kind, flat), or null: a combination k_main's static_asserts exclude.
MainKernel main_kernel(MainKind k, bool flat) {
    for (const MainRow& r : main_kernels())
        if (r.kind.mode == k.mode && r.kind.flavour == k.flavour && r.kind.route == k.route && r.flat == flat) return r.fn;
    return nullptr;
}

// Blocks of a persistent launch: `per_block` work items each, `per_cu` per CU at the most; `reserve_cus` CUs stay free for collectives.
int persistent_grid(const pf_handle* h, long ntasks, int per_block, int per_cu) {
    const int cus = std::max(1, h->prop.multiProcessorCount - (h->reducing ? h->reserve_cus : 0));
    return (int)std::max<long>(1, std::min<long>((long)per_cu * cus, (ntasks + per_block - 1) / per_block));
}

// One k_main launch, one work item per 32-token tile (a routed launch sizes its grid from the same upper bound: the device
// knows the real count).  timed: its own pair of events, "main" or for MODE_FIRST "embed"; else the caller brackets it.
int launch_main(pf_handle* h, MainKind kind, const MainArgs& a, bool timed) {
    const MainKernel fn = main_kernel(kind, kind.route == ROUTE_COMPACT || a.flat);   // (the compact tiling is its own)
    if (!fn) return fail(h, PF_ESTATE, "no k_main for mode %d, flavour %d, route %d", kind.mode, kind.flavour, kind.route);
    const int grid = persistent_grid(h, (long)a.B * a.nt_aln, MAIN_WAVES, 1);
    ProfScope ps(h, kind.mode == MODE_FIRST ? K_EMBED : K_MAIN, timed);
    hipLaunchKernelGGL(fn, dim3(grid), dim3(MAIN_THREADS), MAIN_LDS_BYTES, h->cur, a);
    HIPCHK(h, hipGetLastError());
    return PF_OK;
}

// The plan k_main_plan leaves for a run of B alignments, as the host addresses it (pf_layout.h, above main_plan_ints).
struct MainPlan { const int *nf, *ns, *flist, *slist, *cpre; };
MainPlan main_plan(const int* plan, int B) { return {&plan[0], &plan[1], &plan[4], &plan[4 + B], &plan[4 + 2 * B]}; }

// The split route's statistics (option "stats_dedup", pf_device.hip.h above k_row_stats).  How a run of Lloc sites goes:
//   ROWS      k_row_stats alone: the shape and the routing rule (main_dedup_max_k) show that no split alignment can have
//             more than ROW_STATS_KMAX distinct columns - 60 x 500 at option 1: at most 425
//   ROWS_BIG  k_row_stats, and the statistics launch over the alignments beyond it (k_stats_plan lists them once per run)
//   LAUNCH    the statistics launch over the whole split list: option 0, or more sites than k_row_stats' map holds (such
//             a run has no classes: every K = Lloc)
enum { STATS_ROWS, STATS_ROWS_BIG, STATS_LAUNCH };
int split_stats_form(const pf_handle* h, int Lloc) {
    if (!h->stats_dedup || Lloc > ROW_STATS_MAP_SITES) return STATS_LAUNCH;
    return std::min(Lloc, main_dedup_max_k(Lloc, h->main_dedup)) <= ROW_STATS_KMAX ? STATS_ROWS : STATS_ROWS_BIG;
}
// (the list k_stats_plan leaves: count | alignments, in outpart - written by the last block only, behind every statistics launch)
int* stats_big_list(float* outpart) { return reinterpret_cast<int*>(outpart); }

// c: the compact launch's arguments (the split list).  Under the debug taps x of the repeated sites is filled in behind
// k_row_stats, as the statistics launch does for its alignments.
int launch_split_stats(pf_handle* h, const MainArgs& c) {
    const int form = split_stats_form(h, c.Lloc);
    if (form == STATS_LAUNCH) return launch_main(h, {MODE_STATS, PLAIN, ROUTE_LIST}, c, false);
    hipLaunchKernelGGL(k_row_stats, dim3(persistent_grid(h, (long)c.B * c.P, 1, 1)), dim3(ROW_STATS_THREADS), ROW_STATS_LDS_BYTES, h->cur, c);
    HIPCHK(h, hipGetLastError());
    if (c.store_x_last) {
        hipLaunchKernelGGL(k_copy_repeats, dim3(persistent_grid(h, (long)c.B * c.P * c.Lloc * 16, 256, 8)), dim3(256), 0, h->cur, c);
        HIPCHK(h, hipGetLastError());
    }
    if (form == STATS_ROWS) return PF_OK;
    MainArgs s = c;
    s.acount = stats_big_list(c.outpart); s.alist = s.acount + 1;
    return launch_main(h, {MODE_STATS, PLAIN, ROUTE_LIST}, s, false);
}

// One block's k_main work of a run whose alignments are routed (option "main_dedup"): the fused launch over the
// alignments that stay on it, and for the others the compact launch followed by what must see every site in place - the
// statistics launch, or after the last block the head sums.  Each returns at once where its list is empty.
int launch_main_routed(pf_handle* h, int mode, const MainArgs& m, const MainPlan& p) {
    int rc;
    MainArgs f = m, c = m;              // the fused launch's; the compact launch's and its followers'
    f.acount = p.nf; f.alist = p.flist;
    if ((rc = launch_main(h, {mode, PLAIN, ROUTE_LIST}, f, false))) return rc;
    c.acount = p.ns; c.alist = p.slist; c.cpre = p.cpre;
    c.term = m.spart; c.prof = nullptr; // (spart: dead since k_rowfin read it)
    if ((rc = launch_main(h, {mode, PLAIN, ROUTE_COMPACT}, c, false))) return rc;
    if (mode != MODE_LAST && mode != MODE_LAST_FOLD) return launch_split_stats(h, c);
    hipLaunchKernelGGL(main_kernel({HEAD_PARTS, PLAIN, ROUTE_LIST}, m.flat != 0), dim3(persistent_grid(h, (long)m.B * m.nt_aln, 4, 8)),
                       dim3(256), 0, h->cur, c);
    HIPCHK(h, hipGetLastError());
    return PF_OK;
}

// ---- the forward pass as phases over one shard's workspace -------------------------------------
// Row statistics feeding a block: `nparts` partial sums of 72 floats per pair (k_main leaves one per tile,
// k_embed and the reduced / all-reduced form one).
struct RowStats { const float* p; int nparts; int flat; };   // flat: k_main's per-part slots (part_range) instead of
                                                            // nparts consecutive partials per pair
// An empty shard (Lloc = 0: a rank of L_total < world) launches no kernel; where its kernels would leave row
// statistics or site sums it leaves zeros, its share of every sum.
struct ShardRun {
    Workspace w;
    const uint8_t* d_idx;
    float* d_out;
    int B, N, P, Lloc, L_total;
    TilePlan tp;       // k_main's tiling of (P, Lloc), computed once per run
    hipStream_t stream;    // the stream the run's launches go to
    RowStats rs;           // where the next block's row statistics are
    float* d_smap = nullptr;   // [B][P][Lloc] site map of the head's terms (pf_forward_site_map*), or null
    const float* d_w = nullptr;     // weighted forwards (unsharded): site weights [B][Lloc] and what k_weight_sums made
    const float* d_wst = nullptr;   // of them, [B][4] (pf_weights.hip.h); null: an unweighted forward
    bool routed = false;            // option "main_dedup": w.plan holds the alignments' routes (forward_chunk decides)
};

int zero_fill(pf_handle* h, float* p, size_t n) {
    HIPCHK(h, hipMemsetAsync(p, 0, n * sizeof(float), h->cur));
    return PF_OK;
}

MainArgs main_args(pf_handle* h, const ShardRun& r) {
    MainArgs m{};
    m.x = r.w.x; m.qrow = r.w.qrow; m.qcol = r.w.qcol;
    m.mfrag = reinterpret_cast<const frag_t*>(r.w.mfrag); m.rq = r.w.rq; m.ctx = r.w.ctx; m.spart = r.w.spart;
    m.outpart = r.w.outpart; m.table = h->table; m.idx = r.d_idx; m.pair_i = h->pair_i; m.pair_j = h->pair_j;
    m.B = r.B; m.N = r.N; m.P = r.P; m.Lloc = r.Lloc;
    m.flat = r.tp.flat; m.nt_aln = r.tp.nt_aln; m.slots_aln = r.tp.slots_aln;
    m.store_x_last = h->debug_keep ? 1 : 0;
    m.trash_tok = (size_t)r.B * r.P * r.Lloc;
    m.ablate = h->ablate;
    m.prof = h->phase_prof_last ? nullptr : h->phase_prof;
    m.w = r.d_w;
    m.srep = r.w.srep;
    m.ulist = r.w.ulist; m.ucount = r.w.ucount;
    return m;
}

// Block 0's consumers (k_colstats, k_main) form x0 = T[a_i] + T[a_j] themselves unless the round-1 path is
// requested; the MFMA cross-check kernels and single-block models keep the materialised x0.
bool x0_on_the_fly(const pf_handle* h) {
    return !h->materialize_x0 && !h->embed_mfma && h->n_blocks > 1;
}

// k_main's work once per distinct column (option "main_dedup"): forwards on block 0's on-the-fly x0, site-sharded and
// emulated ranks included - a rank routes from the classes of its own site range, its partials feed the same sums;
// weighted and site-map forwards keep the fused launch.
bool routes_main(const pf_handle* h, const ShardRun& r) {
    return h->main_dedup != 0 && !r.d_smap && !r.d_w && x0_on_the_fly(h) && r.Lloc > 0;
}

// A run of B alignments over Lloc of L_total sites, on the main stream, its workspace still to be laid out.
ShardRun shard_run(const pf_handle* h, const uint8_t* d_idx, float* d_out, int B, int N, int Lloc, int L_total,
                   float* d_smap = nullptr, const float* d_w = nullptr, const float* d_wst = nullptr) {
    ShardRun r{};
    r.d_idx = d_idx; r.d_out = d_out; r.d_smap = d_smap; r.d_w = d_w; r.d_wst = d_wst;
    r.B = B; r.N = N; r.P = N * (N - 1) / 2; r.Lloc = Lloc; r.L_total = L_total;
    r.tp = tile_plan(h, r.P, Lloc); r.stream = h->stream; r.routed = routes_main(h, r);
    return r;
}

// The classes of equal columns of B alignments (k_site_classes), in front of everything that reads them: once per forward -
// the indices change from call to call.  Option site_dedup = 0: the identity map, same kernels.  With `plan`, the routes of
// k_main's work over P pairs follow on the device (k_main_plan, option "main_dedup"), inside the same pair of events.
int launch_site_classes(pf_handle* h, const SiteClassArgs& a, int B, int* plan = nullptr, int P = 0, int* stats_big = nullptr) {
    if (!a.Lloc) return PF_OK;
    ProfScope ps(h, K_SITE_CLASSES);
    hipLaunchKernelGGL(k_site_classes, dim3(B), dim3(SC_THREADS), 0, h->cur, a);
    HIPCHK(h, hipGetLastError());
    if (!plan) return PF_OK;
    hipLaunchKernelGGL(k_main_plan, dim3(1), dim3(64), 0, h->cur, a.ucount, plan, B, P, a.Lloc, h->main_dedup);
    HIPCHK(h, hipGetLastError());
    if (!stats_big) return PF_OK;
    hipLaunchKernelGGL(k_stats_plan, dim3(1), dim3(64), 0, h->cur, a.ucount, plan, stats_big, B);
    HIPCHK(h, hipGetLastError());
    return PF_OK;
}

// Debug taps of what launch_site_classes left for the run (raw int32 bits in the float taps): "srep" and "ulist"
// [B][Lloc] (ulist: the first ucount[b] entries of a row are written), "ucount" [B], and for a routed run "plan"
// (pf_layout.h, main_plan_ints) - a run that is not routed leaves no "plan" tap behind.
int save_route_taps(pf_handle* h, const ShardRun& r) {
    if (!r.Lloc) return PF_OK;
    const size_t nsite = (size_t)r.B * r.Lloc;
    int rc;
    if ((rc = save_tap(h, "srep", reinterpret_cast<const float*>(r.w.srep), nsite))) return rc;
    if ((rc = save_tap(h, "ulist", reinterpret_cast<const float*>(r.w.ulist), nsite))) return rc;
    if ((rc = save_tap(h, "ucount", reinterpret_cast<const float*>(r.w.ucount), (size_t)r.B))) return rc;
    if (r.routed) return save_tap(h, "plan", reinterpret_cast<const float*>(r.w.plan), (size_t)main_plan_ints(r.B));
    h->taps.erase("plan");
    return PF_OK;
}

// embedding + pair expansion + row statistics of block 0
int phase_first(pf_handle* h, const ShardRun& r) {
    if (!r.Lloc) return zero_fill(h, r.w.srow, (size_t)r.B * r.P * SROW);
    int rc;
    if (h->embed_mfma) {
        MainArgs m = main_args(h, r);
        m.wimg = reinterpret_cast<const frag_t*>(h->first_img); m.consts = h->first_consts;
        m.wv_lo = reinterpret_cast<const frag_t*>(h->blk[0].wv_lo);
        if ((rc = launch_main(h, {MODE_FIRST}, m, true))) return rc;
    } else {
        // x0 is written only for those who read it: the round-1 consumers or the "x0" debug tap
        float* x0 = (x0_on_the_fly(h) && !h->debug_keep) ? nullptr : r.w.x;
        EmbedArgs e{r.d_idx, h->pair_i, h->pair_j, h->pair_table, h->table, x0, r.w.qrow, r.w.srow,
                    r.B, r.N, r.P, r.Lloc, h->bad_idx_dev, r.d_w};
        const int ntasks = r.B * r.P, wpb = EMBED_THREADS / 64;
        const int grid = std::max(1, std::min(h->prop.multiProcessorCount, (ntasks + wpb - 1) / wpb));
        ProfScope ps(h, K_EMBED);
        if (r.d_w) hipLaunchKernelGGL(k_embed<true>, dim3(grid), dim3(EMBED_THREADS), EMBED_LDS_BYTES, h->cur, e);
        else hipLaunchKernelGGL(k_embed<false>, dim3(grid), dim3(EMBED_THREADS), EMBED_LDS_BYTES, h->cur, e);
        HIPCHK(h, hipGetLastError());
    }
    if (h->debug_keep) return save_tap(h, "x0", r.w.x, (size_t)r.B * r.P * r.Lloc * 64);
    return PF_OK;
}

int tiles_of(int Lloc) { return (Lloc + 31) / 32; }

// per-tile partials -> w.srow (one row per pair): what an all-reduce or a debug tap wants
int launch_rowsum(pf_handle* h, const ShardRun& r, RowStats* rs) {
    if (rs->p == r.w.srow) return PF_OK;             // already one row per pair, in place
    const int n = r.B * r.P * SROW;
    if (!r.Lloc) { *rs = RowStats{r.w.srow, 1, 0}; return zero_fill(h, r.w.srow, n); }
    ProfScope ps(h, K_ROWFIN);
    hipLaunchKernelGGL(k_rowsum, dim3((n + 255) / 256), dim3(256), 0, h->cur, rs->p, r.w.srow, r.B * r.P, rs->nparts,
                       rs->flat, r.P, r.Lloc, r.tp.slots_aln);
    HIPCHK(h, hipGetLastError());
    *rs = RowStats{r.w.srow, 1, 0};
    return PF_OK;
}

// per-tile head sums of the last block -> distances
int launch_outsum(pf_handle* h, const ShardRun& r) {
    const int n = r.B * r.P;
    if (!r.Lloc) return zero_fill(h, r.d_out, n);
    ProfScope ps(h, K_ROWFIN);
    const TilePlan& tp = r.tp;
    hipLaunchKernelGGL(k_outsum, dim3((n + 255) / 256), dim3(256), 0, h->cur, r.w.outpart, r.d_out, n,
                       tiles_of(r.Lloc), 1.0f / (float)r.L_total, tp.flat, r.P, r.Lloc, tp.slots_aln, r.d_wst);
    HIPCHK(h, hipGetLastError());
    return PF_OK;
}

// the per-part statistics a k_main launch leaves in spart
RowStats main_stats(const ShardRun& r) { return RowStats{r.w.spart, tiles_of(r.Lloc), r.tp.flat}; }

// where block 0's statistics are after phase_first: one row per pair from k_embed, per-tile partials from
// the MFMA cross-check path
RowStats first_stats(pf_handle* h, const ShardRun& r) {
    return h->embed_mfma ? main_stats(r) : RowStats{r.w.srow, 1, 0};
}

// row statistics (rs) -> the row-mix matrices / fragments of every pair
int launch_rowfin(pf_handle* h, const ShardRun& r, int k, const RowStats& rs) {
    const BlockDev& d = h->blk[k]; const Workspace& w = r.w;
    RowFinArgs a{rs.p, w.mrow, reinterpret_cast<frag_t*>(w.mfrag), d.row_woT, d.row_bv, d.row_bo, d.col_bo,
                 r.B * r.P, rs.nparts, (float)r.L_total, rs.flat, r.P, r.Lloc, r.tp.slots_aln, 1};
    // enough blocks to fill the chip a few times over (8 x 256-thread blocks per CU), each amortising its
    // out_proj weights over `iters` groups of four pairs
    const int groups = (r.B * r.P + 3) / 4;
    a.iters = std::max(1, std::min(16, groups / (4 * 8 * std::max(1, h->prop.multiProcessorCount))));
    // q' / mean(q') can reach L_total: past 16,384 sites the B side of the row mix is scaled down by a power of
    // two and the base matrix up (pf_device.hip.h, "fp16 operand ranges"); exact, and 1 for every usual shape
    a.b_scale = 1.f;
    for (long lim = 16384; lim < (long)r.L_total && a.b_scale > 1.f / 256.f; lim *= 2) a.b_scale *= 0.5f;
    a.a_scale = 1.f / a.b_scale;
    a.rq = w.rq; a.wst = r.d_wst;     // (wst, weighted: W and the scales per alignment (k_weight_sums) instead)
    ProfScope ps(h, K_ROWFIN);
    hipLaunchKernelGGL(k_rowfin, dim3((groups + a.iters - 1) / a.iters), dim3(256), 0, h->cur, a);
    HIPCHK(h, hipGetLastError());
    return PF_OK;
}

// x (block 0 on the fly: the embedding table), qrow, mrow -> qcol and the column partials, for the first site of every class
int launch_colstats(pf_handle* h, const ShardRun& r, int k) {
    const BlockDev& d = h->blk[k]; const Workspace& w = r.w;
    ColStatsArgs a{w.x, w.qrow, w.mrow, w.qcol, w.part, d.col_wqk, d.col_bqk, d.row_bo, r.B, r.P, r.Lloc, w.G, tiles_of(r.Lloc),
                   w.sub, w.S, w.fine, h->table, r.d_idx, h->pair_i, h->pair_j, r.N, w.ulist, w.ucount};
    ProfScope ps(h, K_COLSTATS);
    const unsigned nblk = (unsigned)(r.B * a.nchunks * w.nparts());
    void (*fn)(ColStatsArgs) = k_colstats<true, 0, 16>;   // block 0 on the fly; else by the LDS ring or by registers (named in the code object's order)
    if (k != 0 || !x0_on_the_fly(h)) fn = h->colstats_ring ? k_colstats<false, PF_CS_RING, PF_CS_MT> : k_colstats<false, 0, 16>;
    hipLaunchKernelGGL(fn, dim3(nblk), dim3(256), 0, h->cur, a);
    HIPCHK(h, hipGetLastError());
    return PF_OK;
}

// the partials (of the site's class) -> ctx, for every site
int launch_colfin(pf_handle* h, const ShardRun& r, int k) {
    const BlockDev& d = h->blk[k]; const Workspace& w = r.w;
    ColFinArgs a{w.part, w.ctx, d.col_wvT, d.col_bv, r.B, r.Lloc, w.G, (float)r.P, r.P, w.sub, w.S, w.fine, w.srep};
    ProfScope ps(h, K_COLFIN);
    hipLaunchKernelGGL(k_colfin, dim3(r.B * r.Lloc), dim3(COLFIN_THREADS), 0, h->cur, a);
    HIPCHK(h, hipGetLastError());
    return PF_OK;
}

// Every kernel on MainArgs: the one place that spells k_main's instantiations.  The rows stand in the order in which the
// code object lists the kernels - a row moved, added or dropped changes it (profiles/forward_driver_refactor.txt).
template <int MODE, bool FLAT, int FLAVOUR = PLAIN, int ROUTE = ROUTE_ALL>
MainRow main_row() { return {{MODE, FLAVOUR, ROUTE}, FLAT, k_main<MODE, FLAT, FLAVOUR == SITEMAP, FLAVOUR == WEIGHTED, ROUTE>}; }
template <bool FLAT>
MainRow head_parts_row() { return {{HEAD_PARTS, PLAIN, ROUTE_LIST}, FLAT, k_head_parts<FLAT>}; }
const std::vector<MainRow>& main_kernels() {
    static const std::vector<MainRow> rows = {
        // routed blocks: the fused list launch (flat, by rows), the compact launch, and what follows the first of them
        main_row<MODE_MID0, true, PLAIN, ROUTE_LIST>(), main_row<MODE_MID0, false, PLAIN, ROUTE_LIST>(), main_row<MODE_MID0, true, PLAIN, ROUTE_COMPACT>(),
        main_row<MODE_STATS, true, PLAIN, ROUTE_LIST>(), main_row<MODE_STATS, false, PLAIN, ROUTE_LIST>(), head_parts_row<true>(), head_parts_row<false>(),
        main_row<MODE_MID, true, PLAIN, ROUTE_LIST>(), main_row<MODE_MID, false, PLAIN, ROUTE_LIST>(), main_row<MODE_MID, true, PLAIN, ROUTE_COMPACT>(),
        main_row<MODE_LAST, true, PLAIN, ROUTE_LIST>(), main_row<MODE_LAST, false, PLAIN, ROUTE_LIST>(), main_row<MODE_LAST, true, PLAIN, ROUTE_COMPACT>(),
        main_row<MODE_LAST_FOLD, true, PLAIN, ROUTE_LIST>(), main_row<MODE_LAST_FOLD, false, PLAIN, ROUTE_LIST>(), main_row<MODE_LAST_FOLD, true, PLAIN, ROUTE_COMPACT>(),
        // every alignment of the run, by rows and flat: plain, with the head's site map (last block only), with site weights
        main_row<MODE_FIRST, false>(), main_row<MODE_MID, false>(), main_row<MODE_MID0, false>(), main_row<MODE_LAST, false>(), main_row<MODE_LAST_FOLD, false>(),
        main_row<MODE_FIRST, true>(), main_row<MODE_MID, true>(), main_row<MODE_MID0, true>(), main_row<MODE_LAST, true>(), main_row<MODE_LAST_FOLD, true>(),
        main_row<MODE_LAST, false, SITEMAP>(), main_row<MODE_LAST_FOLD, false, SITEMAP>(), main_row<MODE_LAST, true, SITEMAP>(), main_row<MODE_LAST_FOLD, true, SITEMAP>(),
        main_row<MODE_MID, false, WEIGHTED>(), main_row<MODE_MID0, false, WEIGHTED>(), main_row<MODE_LAST, false, WEIGHTED>(), main_row<MODE_LAST_FOLD, false, WEIGHTED>(),
        main_row<MODE_MID, true, WEIGHTED>(), main_row<MODE_MID0, true, WEIGHTED>(), main_row<MODE_LAST, true, WEIGHTED>(), main_row<MODE_LAST_FOLD, true, WEIGHTED>(),
    };
    return rows;
}

// Which k_main launch block k of a run is, and whether it goes by the run's routes.
struct BlockKind { MainKind kind; bool routed; };
BlockKind block_kind(const pf_handle* h, const ShardRun& r, int k) {
    const bool last = k + 1 >= h->n_blocks;
    const MainKind kind{!last ? (k == 0 && x0_on_the_fly(h) ? MODE_MID0 : MODE_MID) : (h->head_fold ? MODE_LAST_FOLD : MODE_LAST),
                        r.d_w ? WEIGHTED : (r.d_smap && last) ? SITEMAP : PLAIN};
    // (under the debug taps the full last block also writes x of every site: all alignments through the fused launch)
    return {kind, r.routed && !(kind.mode == MODE_LAST && h->debug_keep)};
}

// row + column attention applied, FFN, the next block's row statistics or the head's sums
int launch_block_main(pf_handle* h, const ShardRun& r, int k) {
    const BlockKind b = block_kind(h, r, k);
    const bool last = k + 1 >= h->n_blocks;
    MainArgs m = main_args(h, r);
    m.wimg = reinterpret_cast<const frag_t*>(h->blk[k].wimg); m.consts = h->blk[k].consts;
    m.wv_lo = last ? nullptr : reinterpret_cast<const frag_t*>(h->blk[k + 1].wv_lo);
    if (last) { m.sitemap = r.d_smap; if (h->phase_prof_last) m.prof = h->phase_prof; }
    // a routed run's two or three launches per block stand between ONE pair of events: pf_profile_get("main") keeps
    // counting one launch per block and run, its time is the block's
    ProfScope ps(h, K_MAIN, r.routed);
    int rc = b.routed ? launch_main_routed(h, b.kind.mode, m, main_plan(r.w.plan, r.B)) : launch_main(h, b.kind, m, !r.routed);
    if (rc || b.kind.mode != MODE_LAST_FOLD || !h->debug_keep) return rc;
    // the folded head never forms the last x: the full FFN writes it for the tap (in place, after the folded launch
    // has read its input), its head sums go to spart, dead since k_rowfin - the distances stay the folded ones
    m.outpart = r.w.spart; m.prof = nullptr;
    return launch_main(h, {MODE_LAST, r.d_w ? WEIGHTED : PLAIN}, m, !r.routed);
}

// block k given its row statistics (already reduced over ranks in a site-sharded run)
int phase_block(pf_handle* h, const ShardRun& r, int k, RowStats rs) {
    if (!r.Lloc) return PF_OK;
    const std::string tag = std::to_string(k);
    const size_t pairs = (size_t)r.B * r.P, sites = (size_t)r.B * r.Lloc;
    int rc;
    if (h->debug_keep && ((rc = launch_rowsum(h, r, &rs)) || (rc = save_tap(h, "srow" + tag, rs.p, pairs * SROW)))) return rc;
    if ((rc = launch_rowfin(h, r, k, rs))) return rc;
    if ((rc = launch_colstats(h, r, k))) return rc;
    if ((rc = launch_colfin(h, r, k))) return rc;
    if (h->debug_keep && ((rc = save_tap(h, "ctx" + tag, r.w.ctx, sites * 64)) || (rc = save_tap(h, "mrow" + tag, r.w.mrow, pairs * MROW)))) return rc;
    if ((rc = launch_block_main(h, r, k))) return rc;
    // (q' of the next block's row attention, per token: what the statistics phase stored beside its partial sums)
    if (h->debug_keep && k + 1 < h->n_blocks && (rc = save_tap(h, "qrow" + std::to_string(k + 1), r.w.qrow, pairs * r.Lloc * 4))) return rc;
    if (h->debug_keep) return save_tap(h, "x" + std::to_string(k + 1), r.w.x, pairs * r.Lloc * 64);
    return PF_OK;
}

// Does this forward issue collectives?  Only the site-sharded entry points on a handle with a communicator.
bool reduces_now(const pf_handle* h) { return h->sharded_call && (h->world > 1 || h->comm[0]); }
// A site-sharded call for an empty site range on a handle whose forward communicates: the rank holds no token
// but must still join every collective of its peers.
bool empty_rank_call(const pf_handle* h, int Lloc) { return Lloc == 0 && reduces_now(h); }

// How a chunk of B alignments is cut for the overlapped schedule: two halves when collectives run.  Every
// rank must cut identically (one all-reduce sequence per half), so this depends on B and the options only.
int halves_of(const pf_handle* h, int B) {
    if (B < 2 || h->debug_keep) return 1;       // debug taps are kept per name: the whole chunk in one piece
    if (reduces_now(h)) return h->overlap ? 2 : 1;   // (every rank sets the same options, so all cut alike)
    return h->two_streams ? 2 : 1;
}

int ensure_second_stream(pf_handle* h) {
    if (h->stream2) return PF_OK;
    HIPCHK(h, hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    return PF_OK;
}

// Whatever way a forward leaves - a HIPCHK return included - the handle goes back to its main stream and stops
// reserving CUs for collectives (an early return used to leave `reducing` / `cur` set).
struct ForwardScope {
    pf_handle* h;
    ForwardScope(pf_handle* h_, bool reduces) : h(h_) { h->reducing = reduces; }
    ~ForwardScope() { h->cur = h->stream; h->reducing = false; }
};

// The schedule of the default kernels over one rank's runs - the one or two half-batches of a chunk, each on its own
// stream - or over every emulated rank's in rank order.  reduce(site_sums) stands in for the all-reduce of the row
// statistics (false: it leaves every run's `rs` at the reduced sums) or of the site sums (true: into the buffer the
// caller reads); without collectives it does nothing and k_rowfin reads the per-tile partials directly.
template <class Reduce>
int schedule(pf_handle* h, ShardRun* runs, size_t nruns, Reduce reduce) {
    ShardRun* const end = runs + nruns;
    int rc;
    for (ShardRun* r = runs; r != end; ++r) {
        h->cur = r->stream;
        const SiteClassArgs sc{r->d_idx, r->w.srep, r->w.ulist, r->w.ucount, r->N, r->Lloc, h->site_dedup ? 1 : 0};
        // (a routed run that may hold alignments beyond k_row_stats: their list, for the statistics launch)
        int* const big = r->routed && split_stats_form(h, r->Lloc) == STATS_ROWS_BIG ? stats_big_list(r->w.outpart) : nullptr;
        if ((rc = launch_site_classes(h, sc, r->B, r->routed ? r->w.plan : nullptr, r->P, big))) return rc;
        if (h->debug_keep && (rc = save_route_taps(h, *r))) return rc;
        if ((rc = phase_first(h, *r))) return rc;
        r->rs = first_stats(h, *r);
    }
    for (int k = 0; k < h->n_blocks; ++k) {
        if ((rc = reduce(false))) return rc;
        for (ShardRun* r = runs; r != end; ++r) {
            h->cur = r->stream;
            if ((rc = phase_block(h, *r, k, r->rs))) return rc;
            r->rs = main_stats(*r);
        }
    }
    for (ShardRun* r = runs; r != end; ++r) {
        h->cur = r->stream;
        if ((rc = launch_outsum(h, *r))) return rc;
    }
    return reduce(true);
}

// One batch chunk, everything resident on the device.
// Site-sharded runs with >= 2 alignments are cut into two half-batches on two streams: the all-reduce of one
// half (RCCL kernels on a few CUs; the persistent compute kernels leave `reserve_cus` free) runs beside the
// column statistics / FFN of the other.  Each half is an independent forward, so the results are those of
// the serial schedule bit for bit; the collectives double in number (2 x (n_blocks + 1)) and halve in size.
// Single-GPU forwards are cut the same way (option "two_streams"): the halves run free, and whichever is in a
// kernel tail, a small kernel or a launch gap leaves its CUs to the other.  An empty rank (Lloc = 0) cuts and
// reduces exactly as its peers do.
// d_smap (site-map entry points, unsharded): the chunk's [B][P][Lloc] map of head terms, written by the last block.
// d_w, d_wst (weighted forwards, unsharded): the chunk's weight rows [B][Lloc] and their sums [B][4].
int forward_chunk(pf_handle* h, const uint8_t* d_idx, int B, int N, int Lloc, int L_total, float* d_out,
                  float* d_smap = nullptr, const float* d_w = nullptr, const float* d_wst = nullptr) {
    const int P = N * (N - 1) / 2;
    const bool reduces = reduces_now(h);
    const int nh = halves_of(h, B);
    int rc = ensure_pairs(h, N);
    if (rc) return rc;
    ShardRun r[2]{};
    int b0 = 0;
    for (int i = 0; i < nh; ++i) {
        const int nb = (nh == 2) ? (i == 0 ? (B + 1) / 2 : B / 2) : B;
        r[i] = shard_run(h, d_idx + (size_t)b0 * N * Lloc, d_out + (size_t)b0 * P, nb, N, Lloc, L_total,
                         d_smap ? d_smap + (size_t)b0 * P * Lloc : nullptr, d_w ? d_w + (size_t)b0 * Lloc : nullptr,
                         d_w ? d_wst + (size_t)b0 * pfw::WST : nullptr);
        if ((rc = ensure_workspace(h, nb, P, Lloc, &r[i].w, i == 1))) return rc;
        b0 += nb;
    }
    ForwardScope scope(h, reduces);
    if (nh == 2) {
        if ((rc = ensure_second_stream(h))) return rc;
        r[1].stream = h->stream2;
        HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));          // inputs were produced on the main stream
        HIPCHK(h, hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
    }
    auto reduce = [&](bool site_sums) -> int {                        // site-sharded runs only
        if (!reduces) return PF_OK;
        for (ShardRun* q = r; q != r + nh; ++q) {                         // each half on its own stream and communicator
            h->cur = q->stream;
            if (!site_sums && (rc = launch_rowsum(h, *q, &q->rs))) return rc;
            if ((rc = allreduce(h, site_sums ? q->d_out : q->w.srow, (size_t)q->B * P * (site_sums ? 1 : SROW)))) return rc;
        }
        return PF_OK;
    };
    if ((rc = schedule(h, r, nh, reduce))) return rc;
    if (nh == 2) {
        HIPCHK(h, hipEventRecord(h->ev_join, h->stream2));         // the caller continues on the main stream
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_join, 0));
    }
    return PF_OK;
}

// Shard emulation's common part (pf_forward_shards_emulated and its float64 twin): the site ranges of
// phyloformer_amd/dist.py::site_range, each non-empty shard's idx[b][n][lo:hi] uploaded (an empty shard contributes
// zeros to every sum and is skipped), and on every exit a stream sync, the device allocations freed and debug_keep,
// off while emulating, restored.
struct ShardStage {
    struct Shard { int Lloc; const uint8_t* d_idx; };
    pf_handle* h;
    const bool keep;
    std::vector<void*> allocs;
    std::vector<Shard> shards;
    explicit ShardStage(pf_handle* h_) : h(h_), keep(h_->debug_keep) { h->debug_keep = false; }
    ShardStage(const ShardStage&) = delete;
    ~ShardStage() {
        hipStreamSynchronize(h->stream);
        for (void* p : allocs) hipFree(p);
        h->debug_keep = keep;
    }
    void* alloc(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return nullptr;
        allocs.push_back(p);
        return p;
    }
    int upload(const uint8_t* idx, int B, int N, int L, int nshards) {
        const int step = (L + nshards - 1) / nshards;
        for (int s = 0; s < nshards; ++s) {
            const int lo = std::min(s * step, L), hi = std::min((s + 1) * step, L);
            if (hi <= lo) continue;
            const int Lloc = hi - lo;
            uint8_t* di = (uint8_t*)alloc((size_t)B * N * Lloc);
            if (!di) return fail(h, PF_ENOMEM, "shard workspace allocation failed");
            std::vector<uint8_t> local((size_t)B * N * Lloc);
            for (int b = 0; b < B; ++b)
                for (int n = 0; n < N; ++n)
                    std::memcpy(&local[((size_t)b * N + n) * Lloc], &idx[((size_t)b * N + n) * L + lo], Lloc);
            if (hipMemcpy(di, local.data(), local.size(), hipMemcpyHostToDevice) != hipSuccess) return fail(h, PF_EHIP, "idx upload failed");
            shards.push_back({Lloc, di});
        }
        return PF_OK;
    }
};

// The one rule for the three grow-only workspaces: ws / ws2 (default kernels) and wsp (float64 paths) together stay
// inside "ws_limit_mb" (or inside the grower's own need, if that is larger).  Called before a forward lays out its
// workspace - a float64 one (`f64`) that has to regrow wsp to `need` bytes, or a default-path one whose chunk takes
// `need` bytes of ws + ws2 - whichever path runs next releases what the other left behind: a handle that alternates
// large default-path and large float64 shapes would otherwise hold twice the budget.  On the default
// side ws / ws2 themselves go too when they alone exceed the budget (a one-stream call may have left `ws` sized for a
// whole chunk that now runs as two halves).
int make_room(pf_handle* h, bool f64, size_t need) {
    const size_t budget = std::max(need, (size_t)h->ws_limit_bytes);
    if (f64 && h->wsp) { HIPCHK(h, hipStreamSynchronize(h->stream)); h->wsp.release(); }   // regrown by the caller
    if (h->ws.cap + h->ws2.cap + (f64 ? need : h->wsp.cap) <= budget) return PF_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->stream2) HIPCHK(h, hipStreamSynchronize(h->stream2));
    if (!f64) {
        h->wsp.release();
        if (h->ws.cap + h->ws2.cap <= budget) return PF_OK;
    }
    h->ws.release(); h->ws2.release();
    return PF_OK;
}

#include "pf_f64_host.hip.h"

// What every entry point refuses.  An empty site range (Lloc = 0) is allowed only to a rank that joins its peers'
// collectives, and it refuses what they refuse - before any collective, so that no peer is left waiting.
int check_dims(pf_handle* h, int B, int N, int Lloc, int L_total) {
    if (!h) return PF_EINVAL;
    if (h->n_blocks == 0) return fail(h, PF_ESTATE, "handle was created without Phyloformer weights (pf_create_bare)");
    if (B < 1 || N < 2 || Lloc < (empty_rank_call(h, Lloc) ? 0 : 1) || L_total < std::max(Lloc, 1))
        return fail(h, PF_EINVAL, "bad dimensions B=%d N=%d L=%d (L_total=%d)", B, N, Lloc, L_total);
    if (h->max_seqs > 0 && N > h->max_seqs)
        // same condition and wording as adaptable_seq2pair, phyloformer/model.py:24-28
        return fail(h, PF_EINVAL, "n_seqs must be smaller or equal to %lld (or pre-compute a larger global_seq2pair)",
                    (long long)h->max_seqs);
    if (N > 32767) return fail(h, PF_EINVAL, "n_seqs %d exceeds the pair-table index range", N);
    return PF_OK;
}

// Alignments per chunk under the workspace budget ("ws_limit_mb").  A chunk of cb alignments lives in `ws`
// (ceil(cb / 2) alignments when it runs as two halves, else all cb) plus `ws2` (floor(cb / 2)); the per-alignment
// size uses the column-statistics plan that will really be used (run-sized blocks can mean hundreds of partial
// buffers per alignment, not the 32 of a whole-group walk).  Every rank derives the same number: it depends on
// the shape, the options and the largest shard only.
size_t chunk_bytes(const pf_handle* h, int cb, int P, int Lloc) {
    const int nh = halves_of(h, cb);
    const int b0 = nh == 2 ? (cb + 1) / 2 : cb, b1 = nh == 2 ? cb / 2 : 0;
    size_t total = 0;
    for (int nb : {b0, b1}) {
        if (nb < 1) continue;
        Workspace w;
        total += pfspan::measure(workspace_list(h, w, nb, P, Lloc), 256);
    }
    return total;
}

// `extra`: bytes per alignment a chunk holds beside its workspace (the site-map calls' map), 0 for the plain forward.
int chunk_batch(pf_handle* h, int B, int P, int Lloc, size_t extra = 0) {
    // k_main counts tiles in 32 bits
    B = (int)std::min<long>(B, std::max<long>(1, 0x7fffffffL / std::max(1, tile_plan(h, P, Lloc).nt_aln) - 1));
    auto fits = [&](int cb) { return chunk_bytes(h, cb, P, Lloc) + (size_t)cb * extra <= (size_t)h->ws_limit_bytes; };
    if (B <= 1 || fits(B)) return std::max(B, 1);
    int lo = 1, hi = B;                     // largest cb in [1, B) that fits (cb = 1 always runs)
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (fits(mid)) lo = mid; else hi = mid;
    }
    return lo;
}

// One launch of a small kernel on h->stream: go() is its header's launcher (a hipError_t), `kid` its profile slot,
// `name` what a failure calls it.
template <class Go>
int launch_on_stream(pf_handle* h, int kid, const char* name, Go&& go) {
    h->cur = h->stream;
    ProfScope ps(h, kid);
    const hipError_t e = go();
    if (e != hipSuccess) return fail(h, PF_EHIP, "%s launch failed: %s", name, hipGetErrorString(e));
    return PF_OK;
}

// ---- site weights (pf_forward_weighted*, pf_forward_sites_weighted, pf_bootstrap_weighted) ------
// What k_weight_sums makes of the weight rows d_w [B][L] of a call, into the grow-only h->d_wst: asynchronous on
// h->stream, behind whatever read the buffer before.
int launch_weight_sums(pf_handle* h, const float* d_w, int B, int L, const float** d_wst) {
    int rc = h->d_wst.reserve(h, (size_t)B * pfw::WST * sizeof(float));
    if (rc) return rc;
    *d_wst = h->d_wst;
    return launch_on_stream(h, K_WEIGHT_SUMS, "k_weight_sums",
                            [&] { return pfw::launch_weight_sums(h->stream, d_w, h->d_wst, B, L, h->bad_idx_dev + 2); });
}

// What the weighted entry points refuse beside their unweighted twins, before any device work: a handle whose
// communicator has more than one rank (W and the weighted sums are not site-sharded) and the MFMA cross-check embedding.
int check_weighted_handle(pf_handle* h) {
    if (h->world > 1)
        return fail(h, PF_ESTATE, "weighted forwards are not site-sharded: this handle's communicator has %d ranks (use a "
                                  "handle without a communicator)", h->world);
    if (h->embed_mfma) return fail(h, PF_ESTATE, "option embed_mfma has no weighted kernel (set it to 0 for weighted forwards)");
    return PF_OK;
}

// host weights w [rows][K]: every one finite and >= 0, every row's sum W > 0 (and finite); `what` names a row
int check_weights(pf_handle* h, const float* w, size_t rows, int K, const char* what) {
    const int64_t at = pfweights::first_bad_weight(w, rows * (size_t)K);
    if (at >= 0)
        return fail(h, PF_EINVAL, "weight %g of %s %lld, position %lld is negative or not finite", (double)w[at], what,
                    (long long)(at / K), (long long)(at % K));
    for (size_t r = 0; r < rows; ++r) {
        const float W = pfweights::weight_sum(w + r * (size_t)K, K);
        if (!(W > 0.f && W <= 3.402823466e38f))
            return fail(h, PF_EINVAL, "the weights of %s %zu sum to %g: W must be positive and finite", what, r, (double)W);
    }
    return PF_OK;
}

// d_w (weighted forwards, unsharded): site weights [B][Lloc] on the device, or null.
int forward_device_impl(pf_handle* h, const uint8_t* d_idx, int B, int N, int l_begin, int l_end,
                        int L_total, float* d_out, const float* d_w = nullptr) {
    const int Lloc = l_end - l_begin;
    if (h && h->sharded_call && Lloc < L_total && !h->comm[0])
        // a partial site range without a communicator would return partial sums divided by L_total
        return fail(h, PF_ESTATE, "site range [%d, %d) of %d needs a communicator (pf_comm_init) to be reduced",
                    l_begin, l_end, L_total);
    int rc = check_dims(h, B, N, Lloc, L_total);
    if (rc) return rc;
    if (l_begin < 0 || l_end > L_total) return fail(h, PF_EINVAL, "site range [%d, %d) outside [0, %d)", l_begin, l_end, L_total);
    HIPCHK(h, hipSetDevice(h->device));
    const float* d_wst = nullptr;
    if (d_w && (rc = launch_weight_sums(h, d_w, B, Lloc, &d_wst))) return rc;
    if (const F64Path* f = f64_path_of(h, N, L_total))
        return forward_device_f64(h, *f, d_idx, B, N, l_begin, l_end, L_total, d_out, d_w, d_wst);
    const int P = N * (N - 1) / 2;
    // every rank must cut the batch into the same chunks (one all-reduce sequence per chunk), so the
    // chunk size is derived from the largest shard, not from this rank's own (an empty rank has none)
    const int Lmax = std::max(Lloc, h->world > 1 || !Lloc ? (L_total + h->world - 1) / h->world : Lloc);
    const int cb = chunk_batch(h, B, P, Lmax);
    if ((rc = make_room(h, false, chunk_bytes(h, cb, P, Lmax)))) return rc;
    for (int b0 = 0; b0 < B; b0 += cb) {
        const int nbch = std::min(cb, B - b0);
        rc = forward_chunk(h, d_idx + (size_t)b0 * N * Lloc, nbch, N, Lloc, L_total, d_out + (size_t)b0 * P, nullptr,
                           d_w ? d_w + (size_t)b0 * Lloc : nullptr, d_wst ? d_wst + (size_t)b0 * pfw::WST : nullptr);
        if (rc) return rc;
    }
    return PF_OK;
}

// After a stream synchronisation: did a kernel of the forwards since the last check see a residue byte > 21?
// (Only the device entry points can get there: pf_forward / pf_forward_sharded validate on the host first.)
int check_bad_idx(pf_handle* h) {
    if (!h->bad_idx_host) return PF_OK;
    if (h->bad_idx_host[1]) {
        h->bad_idx_host[1] = 0u;
        return fail(h, PF_EINVAL, "a site map passed to pf_gather_sites_device, or a taxon table passed to "
                                  "pf_gather_taxa_device, held an entry outside the source alignment (read as site / row 0; "
                                  "the bytes gathered since the last synchronisation are not those of the map)");
    }
    if (h->bad_idx_host[2]) {
        h->bad_idx_host[2] = 0u;
        return fail(h, PF_EINVAL, "weights passed to pf_forward_weighted_device held a negative or non-finite entry, or an "
                                  "alignment's weights summed to 0 (results of the weighted forwards since the last "
                                  "synchronisation are not valid)");
    }
    if (!*h->bad_idx_host) return PF_OK;
    *h->bad_idx_host = 0u;
    return fail(h, PF_EINVAL, "a residue index outside 0..21 was passed to pf_forward_device / pf_forward_sharded_device "
                              "(treated as 21, '-'; results of the forwards since the last synchronisation are not "
                              "those of a valid alignment)");
}

// residues of a host batch: one branch-free pass the compiler vectorises (an early-exit byte loop cost 0.2 ms per
// batch of 16 x 60 x 500: most of what separated the host-buffer rate from the device-resident one); the offender is
// looked for only if there is one
int check_residues(pf_handle* h, const uint8_t* idx, size_t nidx) {
    unsigned bad = 0;
    for (size_t i = 0; i < nidx; ++i) bad |= (unsigned)(idx[i] >= NA);
    if (bad)
        for (size_t i = 0; i < nidx; ++i)
            if (idx[i] >= NA) return fail(h, PF_EINVAL, "residue index %d at offset %zu is outside 0..21", (int)idx[i], i);
    return PF_OK;
}

// Range re-check (pf_handle::recheck_above) of `count` alignments whose results are in host `out` [count][P], on the
// default kernels' results only.  An alignment whose largest distance exceeds recheck_above, or is not finite, is
// computed again on the float64 kernels: stage(list, k, d_buf) puts the bytes [k][N][Lloc] of the alignments `list`
// into d_buf (on h->stream), which holds `cap` of them; h->d_out must hold cap x P floats.  Every rank of a site-
// sharded call holds the same `out` (the all-reduced site sums through the same kernel), so all of them pick the same
// alignments and issue the same collectives of the float64 forward.
// redo(d_idx, list, k) is that float64 forward of the k staged alignments, distances into h->d_out; an entry point
// that returns more than distances (the site-map calls) replaces the rest of alignments `list` there, together with
// their `out`.
template <class Stage, class Redo>
int range_recheck(pf_handle* h, float* out, int count, int N, int l_begin, int l_end, int L_total, uint8_t* d_buf, size_t cap,
                  Stage&& stage, Redo&& redo) {
    if (h->precise >= 0 || h->recheck_above <= 0.0) return PF_OK;
    const int P = N * (N - 1) / 2;
    const size_t per = (size_t)N * (size_t)(l_end - l_begin);
    std::vector<int> list;
    std::vector<float> res;
    try {           // (nothing may throw across the C ABI)
        for (int b = 0; b < count; ++b) {
            const float* ob = out + (size_t)b * P;
            bool inside = true;
            for (int p = 0; p < P; ++p) inside &= ob[p] <= (float)h->recheck_above;      // (false for NaN)
            if (!inside) list.push_back(b);
        }
        res.resize(std::min(list.size(), cap) * (size_t)P);
    } catch (const std::bad_alloc&) { return fail(h, PF_ENOMEM, "out of host memory in the range re-check"); }
    for (size_t g0 = 0; g0 < list.size(); g0 += cap) {
        const size_t nr = std::min(cap, list.size() - g0);
        int rc;
        if (per && (rc = stage(&list[g0], nr, d_buf))) return rc;
        if ((rc = redo(per ? d_buf : nullptr, &list[g0], nr))) return rc;
        HIPCHK(h, hipMemcpyAsync(res.data(), h->d_out, nr * (size_t)P * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (size_t i = 0; i < nr; ++i) std::memcpy(out + (size_t)list[g0 + i] * P, &res[i * P], (size_t)P * sizeof(float));
    }
    h->rechecked += (int64_t)list.size();
    return PF_OK;
}
template <class Stage>
int range_recheck(pf_handle* h, float* out, int count, int N, int l_begin, int l_end, int L_total, uint8_t* d_buf, size_t cap,
                  Stage&& stage) {
    return range_recheck(h, out, count, N, l_begin, l_end, L_total, d_buf, cap, stage, [&](const uint8_t* d_idx, const int*, size_t k) {
        return forward_device_f64(h, PRECISE_F64, d_idx, (int)k, N, l_begin, l_end, L_total, h->d_out);
    });
}

// weighted (pf_forward_weighted): w float [B][Lloc] rides along - checked, uploaded into the grow-only h->d_w, and
// staged again with the bytes of an alignment the range re-check sends to the float64 kernels.
int forward_host_impl(pf_handle* h, const uint8_t* idx, int B, int N, int l_begin, int l_end,
                      int L_total, float* out, const float* w = nullptr, bool weighted = false) {
    const int Lloc = l_end - l_begin;
    int rc = check_dims(h, B, N, Lloc, L_total);
    if (rc) return rc;
    if (!out || (!idx && Lloc > 0)) return fail(h, PF_EINVAL, "null buffer");
    const size_t nidx = (size_t)B * N * Lloc;
    if ((rc = check_residues(h, idx, nidx))) return rc;
    if (weighted) {
        if (!w) return fail(h, PF_EINVAL, "null buffer");
        if ((rc = check_weights(h, w, (size_t)B, Lloc, "alignment"))) return rc;
        if ((rc = check_weighted_handle(h))) return rc;
    }
    HIPCHK(h, hipSetDevice(h->device));
    const size_t nw = (size_t)B * Lloc * sizeof(float);
    if (weighted) {
        if ((rc = h->d_w.reserve(h, nw))) return rc;
        HIPCHK(h, hipMemcpyAsync(h->d_w, w, nw, hipMemcpyHostToDevice, h->stream));
    }
    const int P = N * (N - 1) / 2;
    if ((rc = h->d_idx.reserve(h, nidx))) return rc;
    const size_t nout = (size_t)B * P * sizeof(float);
    if ((rc = h->d_out.reserve(h, nout))) return rc;
    if (nidx) HIPCHK(h, hipMemcpyAsync(h->d_idx, idx, nidx, hipMemcpyHostToDevice, h->stream));
    const bool default_kernels = !f64_path_of(h, N, L_total);
    rc = forward_device_impl(h, h->d_idx, B, N, l_begin, l_end, L_total, h->d_out, weighted ? h->d_w : nullptr);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(out, h->d_out, nout, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!default_kernels) return PF_OK;
    std::vector<uint8_t> sub;
    std::vector<float> wsub;
    const size_t per = (size_t)N * Lloc;
    auto stage = [&](const int* list, size_t k, uint8_t* d_buf) -> int {
        try { sub.resize(k * per); if (weighted) wsub.resize(k * (size_t)Lloc); }
        catch (const std::bad_alloc&) { return fail(h, PF_ENOMEM, "out of host memory in the range re-check"); }
        for (size_t i = 0; i < k; ++i) std::memcpy(&sub[i * per], idx + (size_t)list[i] * per, per);
        HIPCHK(h, hipMemcpyAsync(d_buf, sub.data(), k * per, hipMemcpyHostToDevice, h->stream));
        if (weighted) {          // the flagged alignments' weight rows, in the same order (everything else is on the host by now)
            for (size_t i = 0; i < k; ++i) std::memcpy(&wsub[i * Lloc], w + (size_t)list[i] * Lloc, (size_t)Lloc * sizeof(float));
            HIPCHK(h, hipMemcpyAsync(h->d_w, wsub.data(), k * (size_t)Lloc * sizeof(float), hipMemcpyHostToDevice, h->stream));
        }
        return PF_OK;
    };
    if (!weighted) return range_recheck(h, out, B, N, l_begin, l_end, L_total, h->d_idx, (size_t)B, stage);
    return range_recheck(h, out, B, N, l_begin, l_end, L_total, h->d_idx, (size_t)B, stage, [&](const uint8_t* d_idx, const int*, size_t k) -> int {
        const float* d_wst = nullptr;
        const int rc2 = launch_weight_sums(h, h->d_w, (int)k, Lloc, &d_wst);
        if (rc2) return rc2;
        return forward_device_f64(h, PRECISE_F64, d_idx, (int)k, N, l_begin, l_end, L_total, h->d_out, h->d_w, d_wst);
    });
}

int launch_resample(pf_handle* h, const uint8_t* d_src, int B, int N, int L, int r_begin, int R, uint64_t seed, uint8_t* d_dst) {
    return launch_on_stream(h, K_RESAMPLE, "k_resample",
                            [&] { return pfb::launch_resample(h->stream, d_src, B, N, L, r_begin, R, seed, d_dst); });
}

// a * b * c as size_t, false on overflow
bool mul_size(size_t a, size_t b, size_t c, size_t* out) {
    size_t t;
    return !__builtin_mul_overflow(a, b, &t) && !__builtin_mul_overflow(t, c, out);
}

// map: device int32 - rows [..][K] of a site table (sites) or window starts [..] (start); sets s_begin .. s_begin + S - 1
int launch_gather(pf_handle* h, const uint8_t* d_src, int B, int N, int L, const int32_t* d_sites, const int32_t* d_start,
                  int s_begin, int S, int K, uint8_t* d_dst) {
    return launch_on_stream(h, K_GATHER, "k_gather_sites", [&] {
        return pfs::launch_gather(h->stream, d_src, B, N, L, d_sites, d_start, s_begin, S, K, d_dst, h->bad_idx_dev + 1);
    });
}

// The one loop of every entry point that forwards alignments DERIVED from resident sources (pf_bootstrap,
// pf_forward_sites, pf_forward_windows and, through TaxonCuts, the taxon-axis calls): source b of idx [B][N][L] has S
// derived alignments of Nd x K (Nd = N for everything that cuts the site axis), and
// fill(d_src, nb, j0, nj, d_dst) builds the derived alignments [j0, j0 + nj) of nb consecutive sources at d_src into
// d_dst [nb][nj][Nd][K] on h->stream (k_resample for the bootstrap, k_gather_sites for site maps, k_gather_taxa for
// taxon subsets).  The B sources are
// uploaded once; the B x S derived alignments run in chunks of the size the forward's own chunking picks for B x S
// alignments of Nd x K (chunk_batch, or the float64 path's), cut to a rectangle - whole sources with all their derived
// alignments, or a run of one source's - so that one fill builds a chunk's bytes in the grow-only h->d_rep; the forward
// then reads them there.  A derived alignment's distances are those of pf_forward on its host-built bytes, bit for bit:
// the forward is batch invariant and routes on (Nd, K) alone.  The caller has checked its own arguments; what
// pf_forward checks is checked here, before any device work.  `what` names the derived alignments in messages.
// Weighted derived alignments (pf_forward_sites_weighted): wfill(nb, j0, nj, d_wdst) writes the same rectangle's weight
// rows float [nb][nj][K] into d_wdst on h->stream - a chunk's live in the grow-only h->d_w - and the forward is the
// weighted one; without wfill nothing changes.
// Resident sources (TaxonCuts, which forwards several shapes and sub-calls from one upload): d_resident holds the B
// sources, checked and uploaded by the caller on h->stream; idx is not read, h->d_idx is neither grown nor written.
template <class Fill, class WFill = std::nullptr_t>
int forward_derived(pf_handle* h, const uint8_t* idx, int B, int N, int L, int S, int Nd, int K, float* out, const char* what,
                    Fill&& fill, WFill&& wfill = nullptr, const uint8_t* d_resident = nullptr) {
    constexpr bool weighted = !std::is_same<typename std::decay<WFill>::type, std::nullptr_t>::value;
    if (!out || (!idx && !d_resident)) return fail(h, PF_EINVAL, "null buffer");
    const int P = Nd * (Nd - 1) / 2;
    size_t nout = 0, nrep = 0;
    if (!mul_size((size_t)B, (size_t)S, (size_t)P * sizeof(float), &nout) || !mul_size((size_t)B, (size_t)S, (size_t)Nd * K, &nrep))
        return fail(h, PF_EINVAL, "B=%d x S=%d %s of %d x %d overflow the address space", B, S, what, Nd, K);
    const size_t nidx = (size_t)B * N * L, per_src = (size_t)N * L, per = (size_t)Nd * K;
    int rc = d_resident ? PF_OK : check_residues(h, idx, nidx);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if (!d_resident && (rc = h->d_idx.reserve(h, nidx))) return rc;
    if ((rc = h->d_out.reserve(h, nout))) return rc;
    if (!d_resident) HIPCHK(h, hipMemcpyAsync(h->d_idx, idx, nidx, hipMemcpyHostToDevice, h->stream));
    const uint8_t* d_all = d_resident ? d_resident : h->d_idx;
    const F64Path* f = f64_path_of(h, Nd, K);
    const int total = (int)std::min<int64_t>((int64_t)B * S, INT32_MAX);
    const int cb = f ? f64_chunk_batch(h, *f, total, P, K) : chunk_batch(h, total, P, K);
    const int spc = cb >= S ? cb / S : 0;                  // whole sources per chunk, or
    const int jpc = spc ? S : cb;                          // derived alignments of one source per chunk
    const size_t cap = spc ? (size_t)spc * S : (size_t)jpc;
    if ((rc = h->d_rep.reserve(h, cap * per))) return rc;
    if (weighted && (rc = h->d_w.reserve(h, cap * (size_t)K * sizeof(float)))) return rc;
    for (int b0 = 0; b0 < B; b0 += std::max(spc, 1))
        for (int j0 = 0; j0 < S; j0 += jpc) {
            const int nb = spc ? std::min(spc, B - b0) : 1, nj = std::min(jpc, S - j0);
            if ((rc = fill(d_all + (size_t)b0 * per_src, nb, j0, nj, h->d_rep))) return rc;
            if constexpr (weighted) { if ((rc = wfill(nb, j0, nj, h->d_w))) return rc; }
            rc = forward_device_impl(h, h->d_rep, nb * nj, Nd, 0, K, K, h->d_out + ((size_t)b0 * S + j0) * P,
                                     weighted ? h->d_w : nullptr);
            if (rc) return rc;
        }
    HIPCHK(h, hipMemcpyAsync(out, h->d_out, nout, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (f) return PF_OK;
    // a flagged derived alignment is rebuilt from the resident source bytes (and its weight row with it)
    auto stage = [&](const int* list, size_t k, uint8_t* d_buf) -> int {
        for (size_t i = 0; i < k; ++i) {
            const int b = list[i] / S, j = list[i] % S;
            int rc2 = fill(d_all + (size_t)b * per_src, 1, j, 1, d_buf + i * per);
            if (rc2) return rc2;
            if constexpr (weighted) { if ((rc2 = wfill(1, j, 1, h->d_w + i * (size_t)K))) return rc2; }
        }
        return PF_OK;
    };
    if constexpr (!weighted) return range_recheck(h, out, B * S, Nd, 0, K, K, h->d_rep, cap, stage);
    return range_recheck(h, out, B * S, Nd, 0, K, K, h->d_rep, cap, stage, [&](const uint8_t* d_buf, const int*, size_t k) -> int {
        const float* d_wst = nullptr;
        const int rc2 = launch_weight_sums(h, h->d_w, (int)k, K, &d_wst);
        if (rc2) return rc2;
        return forward_device_f64(h, PRECISE_F64, d_buf, (int)k, Nd, 0, K, K, h->d_out, h->d_w, d_wst);
    });
}

// pf_bootstrap: the derived alignments are the R replicates of the stream (pf_boot.hip.h), K = L.
int bootstrap_impl(pf_handle* h, const uint8_t* idx, int B, int N, int L, int R, uint64_t seed, float* out) {
    int rc = check_dims(h, B, N, L, L);
    if (rc) return rc;
    if (R < 1) return fail(h, PF_EINVAL, "bootstrap needs R >= 1 replicates (got %d)", R);
    return forward_derived(h, idx, B, N, L, R, N, L, out, "replicates", [&](const uint8_t* d_src, int nb, int r0, int nr, uint8_t* d_dst) {
        return launch_resample(h, d_src, nb, N, L, r0, nr, seed, d_dst);
    });
}

// pf_forward_sites / pf_forward_windows: the derived alignments are the S site sets of a host map - a table
// sites [S][K], or (sites == nullptr) the S windows of K sites, `step` apart, of the window rule - uploaded once into
// the grow-only h->d_map.  Sizes are checked before the map is read or built: a caller's S is not trusted further than
// its own table.
// weighted (pf_forward_sites_weighted): w float [S][K], one weight per table entry, uploaded once into the grow-only
// h->d_wtab; a chunk's weight rows are device-to-device copies of its sets' rows.
int sites_impl(pf_handle* h, const uint8_t* idx, int B, int N, int L, const int32_t* sites, int step, int S, int K, float* out,
               const float* w = nullptr, bool weighted = false) {
    int rc = check_dims(h, B, N, L, L);
    if (rc) return rc;
    if (S < 1) return fail(h, PF_EINVAL, "a site map needs S >= 1 sets (got %d)", S);
    if (K < 1 || K > L) return fail(h, PF_EINVAL, "a site set needs 1 <= K <= L sites (got K=%d, L=%d)", K, L);
    const int P = N * (N - 1) / 2;
    size_t nmap = 0, n = 0;
    if (!mul_size((size_t)B, (size_t)S, (size_t)P * sizeof(float), &n) || !mul_size((size_t)B, (size_t)S, (size_t)N * K, &n) ||
        !mul_size((size_t)S, sites ? (size_t)K : 1, sizeof(int32_t), &nmap))
        return fail(h, PF_EINVAL, "B=%d x S=%d site sets of %d x %d overflow the address space", B, S, N, K);
    if (!out || !idx) return fail(h, PF_EINVAL, "null buffer");
    std::vector<int32_t> start;
    if (sites) {
        const int64_t at = pfsites::first_bad_site(sites, (size_t)S * K, L);
        if (at >= 0)
            return fail(h, PF_EINVAL, "site %d at set %lld, position %lld is outside [0, %d)", (int)sites[at],
                        (long long)(at / K), (long long)(at % K), L);
    } else {
        try { start.resize((size_t)S); }
        catch (const std::bad_alloc&) { return fail(h, PF_ENOMEM, "out of host memory for %d window starts", S); }
        for (int s = 0; s < S; ++s) start[s] = pfsites::window_start(L, K, step, s);
    }
    const int32_t* map = sites ? sites : start.data();
    size_t nwt = 0;
    if (weighted) {
        if (!w) return fail(h, PF_EINVAL, "null buffer");
        if (!mul_size((size_t)S, (size_t)K, sizeof(float), &nwt))
            return fail(h, PF_EINVAL, "B=%d x S=%d site sets of %d x %d overflow the address space", B, S, N, K);
        if ((rc = check_weights(h, w, (size_t)S, K, "set"))) return rc;
        if ((rc = check_weighted_handle(h))) return rc;
    }
    // (what is left - the residues - is refused by forward_derived before its first device call)
    bool uploaded = false;
    auto fill = [&](const uint8_t* d_src, int nb, int j0, int nj, uint8_t* d_dst) -> int {
        if (!uploaded) {
            int rc2 = h->d_map.reserve(h, nmap);
            if (rc2) return rc2;
            HIPCHK(h, hipMemcpyAsync(h->d_map, map, nmap, hipMemcpyHostToDevice, h->stream));
            if (weighted) {
                if ((rc2 = h->d_wtab.reserve(h, nwt))) return rc2;
                HIPCHK(h, hipMemcpyAsync(h->d_wtab, w, nwt, hipMemcpyHostToDevice, h->stream));
            }
            uploaded = true;
        }
        return launch_gather(h, d_src, nb, N, L, sites ? h->d_map : nullptr, sites ? nullptr : h->d_map, j0, nj, K, d_dst);
    };
    if (!weighted) return forward_derived(h, idx, B, N, L, S, N, K, out, "site sets", fill);
    // every source of the rectangle takes the same rows j0 .. j0 + nj - 1 of the table (fill ran first: it is uploaded)
    return forward_derived(h, idx, B, N, L, S, N, K, out, "site sets", fill, [&](int nb, int j0, int nj, float* d_wdst) -> int {
        for (int b = 0; b < nb; ++b)
            HIPCHK(h, hipMemcpyAsync(d_wdst + (size_t)b * nj * K, h->d_wtab + (size_t)j0 * K, (size_t)nj * K * sizeof(float),
                                     hipMemcpyDeviceToDevice, h->stream));
        return PF_OK;
    });
}

// pf_bootstrap_weighted: replicate r of pf_bootstrap's stream as the table of its distinct sites and their counts
// (pfweights::boot_counts), every replicate padded with (site 0, weight 0) to K = padded_sites(max_r distinct_r, L);
// built on the host (R x L draws), forwarded by pf_forward_sites_weighted's path, which routes on (N, K).
int bootstrap_weighted_impl(pf_handle* h, const uint8_t* idx, int B, int N, int L, int R, uint64_t seed, float* out) {
    int rc = check_dims(h, B, N, L, L);
    if (rc) return rc;
    if (R < 1) return fail(h, PF_EINVAL, "bootstrap needs R >= 1 replicates (got %d)", R);
    if (!out || !idx) return fail(h, PF_EINVAL, "null buffer");
    size_t n = 0;
    if (!mul_size((size_t)R, (size_t)L, sizeof(int32_t) * 2, &n))
        return fail(h, PF_EINVAL, "B=%d x R=%d replicates of %d x %d overflow the address space", B, R, N, L);
    std::vector<int32_t> all_sites, all_counts, tab;
    std::vector<int> distinct;
    std::vector<float> wt;
    int K = 0;
    try {
        all_sites.resize((size_t)R * L); all_counts.resize((size_t)R * L); distinct.resize((size_t)R);
        int kmax = 1;
        for (int r = 0; r < R; ++r) {
            distinct[r] = pfweights::boot_counts(L, seed, r, &all_sites[(size_t)r * L], &all_counts[(size_t)r * L]);
            kmax = std::max(kmax, distinct[r]);
        }
        K = pfweights::padded_sites(kmax, L);
        tab.assign((size_t)R * K, 0);
        wt.assign((size_t)R * K, 0.f);
        for (int r = 0; r < R; ++r)
            for (int k = 0; k < distinct[r]; ++k) {
                tab[(size_t)r * K + k] = all_sites[(size_t)r * L + k];
                wt[(size_t)r * K + k] = (float)all_counts[(size_t)r * L + k];
            }
    } catch (const std::bad_alloc&) { return fail(h, PF_ENOMEM, "out of host memory for the tables of %d replicates", R); }
    return sites_impl(h, idx, B, N, L, tab.data(), 0, R, K, out, wt.data(), true);
}

// ---- site-resolved distances (pf_forward_site_map*, pf_forward_site_profile, pf_site_moments_device) ----------------
// The head's terms map[b][p][l] = softplus(logit of pair p at site l) - distance[p] is their mean over l - are kept by
// the last block's launch (k_main<MODE_LAST*, .., SITEMAP>, kg_head with a map pointer) and reduced by pf_sitemap.hip.h.

// se [B][P], profile [B][L] of a device map [B][P][L], asynchronous on h->stream.  The partial column sums live in the
// grow-only h->d_mpart, at most 64 MB of them (or one alignment's): larger batches are reduced in pieces - every
// alignment's bits are its own, wherever a piece starts.
int launch_site_moments(pf_handle* h, const float* d_map, int B, int P, int L, float* d_se, float* d_prof) {
    const size_t per = pfm::part_count(1, P, L) * sizeof(double);
    const int nbc = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(B, 65535), ((size_t)64 << 20) / per));
    int rc = h->d_mpart.reserve(h, (size_t)nbc * per);
    for (int b0 = 0; b0 < B && !rc; b0 += nbc)
        rc = launch_on_stream(h, K_SITE_MOMENTS, "k_site_moments", [&] {
            return pfm::launch_site_moments(h->stream, d_map + (size_t)b0 * P * L, std::min(nbc, B - b0), P, L, h->d_mpart,
                                            d_se + (size_t)b0 * P, d_prof + (size_t)b0 * L);
        });
    return rc;
}

// What the site-map entry points refuse beside what pf_forward refuses, before any device work.
int check_site_call(pf_handle* h, int B, int N, int L, size_t* nmap) {
    int rc = check_dims(h, B, N, L, L);
    if (rc) return rc;
    if (h->world > 1)
        return fail(h, PF_ESTATE, "site maps are not site-sharded: this handle's communicator has %d ranks, and a rank would "
                                  "hold a slice of the map (use a handle without a communicator)", h->world);
    const size_t P = (size_t)N * (N - 1) / 2;
    if (!mul_size((size_t)B, P * (size_t)L, sizeof(float), nmap))
        return fail(h, PF_EINVAL, "a site map of B=%d x %zu pairs x %d sites overflows the address space", B, P, L);
    return PF_OK;
}

// The forward of B resident alignments on the kernels `f` (nullptr: the default ones) that keeps the site map: the
// chunks of pf_forward_device, sized so that a chunk's workspace AND its map stay inside "ws_limit_mb".  d_map
// [B][P][L]: every chunk writes its slice; nullptr: a chunk's map lives in the grow-only h->d_smap.  each(b0, nb, dm)
// follows every chunk on h->stream: dm is the map of alignments [b0, b0 + nb).
template <class Each>
int forward_sitemap_device(pf_handle* h, const F64Path* f, const uint8_t* d_idx, int B, int N, int L, float* d_out,
                           float* d_map, Each&& each) {
    const int P = N * (N - 1) / 2;
    const size_t map_per = (size_t)P * L * sizeof(float);
    int rc, cb;
    if (f) {
        if ((rc = f->prepare(h))) return rc;
        size_t off[F64_BUFS];
        const size_t per = f64_bytes(f->dims(h), 1, P, L, off) + map_per;
        cb = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, (size_t)h->ws_limit_bytes / per));
    } else {
        cb = chunk_batch(h, B, P, L, map_per);
        if ((rc = make_room(h, false, chunk_bytes(h, cb, P, L)))) return rc;
    }
    if (!d_map && (rc = h->d_smap.reserve(h, (size_t)cb * map_per))) return rc;
    for (int b0 = 0; b0 < B; b0 += cb) {
        const int nb = std::min(cb, B - b0);
        float* dm = d_map ? d_map + (size_t)b0 * P * L : h->d_smap;
        const uint8_t* di = d_idx + (size_t)b0 * N * L;
        rc = f ? forward_chunk_f64(h, *f, di, nb, N, L, L, d_out + (size_t)b0 * P, dm)
               : forward_chunk(h, di, nb, N, L, L, d_out + (size_t)b0 * P, dm);
        if (rc) return rc;
        if ((rc = each(b0, nb, dm))) return rc;
    }
    return PF_OK;
}

int site_map_device_impl(pf_handle* h, const uint8_t* d_idx, int B, int N, int L, float* d_out, float* d_map) {
    size_t nmap = 0;
    int rc = check_site_call(h, B, N, L, &nmap);
    if (rc) return rc;
    if (!d_idx || !d_out || !d_map) return fail(h, PF_EINVAL, "null buffer");
    HIPCHK(h, hipSetDevice(h->device));
    return forward_sitemap_device(h, f64_path_of(h, N, L), d_idx, B, N, L, d_out, d_map, [](int, int, float*) { return PF_OK; });
}

// pf_forward_site_map (map given) and pf_forward_site_profile (se and profile given): pf_forward's upload, chunks and
// range re-check; what a chunk leaves beside its distances is its map, copied to the host, or the map's moments.
int site_host_impl(pf_handle* h, const uint8_t* idx, int B, int N, int L, float* out, float* map, float* se, float* profile) {
    size_t nmap = 0;
    int rc = check_site_call(h, B, N, L, &nmap);
    if (rc) return rc;
    if (!out || !idx || (!map && (!se || !profile))) return fail(h, PF_EINVAL, "null buffer");
    const int P = N * (N - 1) / 2;
    const size_t nidx = (size_t)B * N * L, per = (size_t)N * L, tok = (size_t)P * L;
    if ((rc = check_residues(h, idx, nidx))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t nout = (size_t)B * P * sizeof(float), nprof = (size_t)B * L * sizeof(float);
    if ((rc = h->d_idx.reserve(h, nidx))) return rc;
    if ((rc = h->d_out.reserve(h, nout))) return rc;
    if (!map) {
        if ((rc = h->d_se.reserve(h, nout))) return rc;
        if ((rc = h->d_prof.reserve(h, nprof))) return rc;
    }
    HIPCHK(h, hipMemcpyAsync(h->d_idx, idx, nidx, hipMemcpyHostToDevice, h->stream));
    const F64Path* f = f64_path_of(h, N, L);
    rc = forward_sitemap_device(h, f, h->d_idx, B, N, L, h->d_out, nullptr, [&](int b0, int nb, float* dm) -> int {
        if (!map) return launch_site_moments(h, dm, nb, P, L, h->d_se + (size_t)b0 * P, h->d_prof + (size_t)b0 * L);
        HIPCHK(h, hipMemcpyAsync(map + (size_t)b0 * tok, dm, (size_t)nb * tok * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));            // the next chunk writes the same buffer
        return PF_OK;
    });
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(out, h->d_out, nout, hipMemcpyDeviceToHost, h->stream));
    if (!map) {
        HIPCHK(h, hipMemcpyAsync(se, h->d_se, nout, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(profile, h->d_prof, nprof, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (f) return PF_OK;
    std::vector<uint8_t> sub;
    auto stage = [&](const int* list, size_t k, uint8_t* d_buf) -> int {
        try { sub.resize(k * per); }
        catch (const std::bad_alloc&) { return fail(h, PF_ENOMEM, "out of host memory in the range re-check"); }
        for (size_t i = 0; i < k; ++i) std::memcpy(&sub[i * per], idx + (size_t)list[i] * per, per);
        HIPCHK(h, hipMemcpyAsync(d_buf, sub.data(), k * per, hipMemcpyHostToDevice, h->stream));
        return PF_OK;
    };
    // a flagged alignment's map / se / profile leave with its distances (everything else is on the host by now, so the
    // device buffers are reused from their start)
    auto redo = [&](const uint8_t* d_idx, const int* list, size_t k) -> int {
        return forward_sitemap_device(h, &PRECISE_F64, d_idx, (int)k, N, L, h->d_out, nullptr, [&](int b0, int nb, float* dm) -> int {
            if (!map) {
                const int rc2 = launch_site_moments(h, dm, nb, P, L, h->d_se + (size_t)b0 * P, h->d_prof + (size_t)b0 * L);
                if (rc2) return rc2;
            }
            for (int i = 0; i < nb; ++i) {
                const size_t hb = (size_t)list[b0 + i], db = (size_t)(b0 + i);
                if (map) {
                    HIPCHK(h, hipMemcpyAsync(map + hb * tok, dm + (size_t)i * tok, tok * sizeof(float), hipMemcpyDeviceToHost, h->stream));
                } else {
                    HIPCHK(h, hipMemcpyAsync(se + hb * P, h->d_se + db * P, (size_t)P * sizeof(float), hipMemcpyDeviceToHost, h->stream));
                    HIPCHK(h, hipMemcpyAsync(profile + hb * L, h->d_prof + db * L, (size_t)L * sizeof(float), hipMemcpyDeviceToHost, h->stream));
                }
            }
            HIPCHK(h, hipStreamSynchronize(h->stream));
            return PF_OK;
        });
    };
    return range_recheck(h, out, B, N, 0, L, L, h->d_idx, (size_t)B, stage, redo);
}

// ---- the taxon axis (pf_gather_taxa_device, pf_forward_taxa, pf_forward_leave_one_out, pf_loo_stats_device) ---------
// A derived alignment is a list of source ROWS (pf_taxa.hip.h); its distances are pf_forward's of the host-cut rows,
// on the path its own shape (M, L) takes.

// taxa: device int32 [..][M]; sets s_begin .. s_begin + S - 1
int launch_gather_taxa(pf_handle* h, const uint8_t* d_src, int B, int N, int L, const int32_t* d_taxa, int s_begin, int S, int M,
                       uint8_t* d_dst) {
    return launch_on_stream(h, K_GATHER_TAXA, "k_gather_taxa", [&] {
        return pft::launch_gather_taxa(h->stream, d_src, B, N, L, d_taxa, s_begin, S, M, d_dst, h->bad_idx_dev + 1);
    });
}

int launch_loo_stats(pf_handle* h, const float* d_full, const float* d_loo, int B, int N, float* d_infl, float* d_shift, float* d_ctx) {
    return launch_on_stream(h, K_LOO_STATS, "k_loo_taxon / k_loo_pair",
                            [&] { return pft::launch_loo_stats(h->stream, d_full, d_loo, B, N, d_infl, d_shift, d_ctx); });
}

// What every call that forwards S sets of M source rows refuses about the sets, before any device work: what pf_forward
// refuses at their shape (M, L), a communicator of more than one rank, and sizes that overflow.  ntab: the bytes of a
// table [S][M].
int check_taxon_sets(pf_handle* h, int B, int L, int S, int M, size_t* ntab) {
    int rc = check_dims(h, B, M, L, L);
    if (rc) return rc;
    if (h->world > 1)
        return fail(h, PF_ESTATE, "taxon subsets are not site-sharded: this handle's communicator has %d ranks (use a handle "
                                  "without a communicator)", h->world);
    const size_t P = (size_t)M * (M - 1) / 2;
    size_t n = 0;
    if (!mul_size((size_t)B, (size_t)S, P * sizeof(float), &n) || !mul_size((size_t)B, (size_t)S, (size_t)M * L, &n) ||
        !mul_size((size_t)S, (size_t)M, sizeof(int32_t), ntab))
        return fail(h, PF_EINVAL, "B=%d x S=%d taxon sets of %d x %d overflow the address space", B, S, M, L);
    return PF_OK;
}

// What the taxon calls refuse beside what pf_forward refuses at the source's shape (N, L), before any device work.
int check_taxa_call(pf_handle* h, int B, int N, int L, int S, int M, size_t* ntab) {
    int rc = check_dims(h, B, N, L, L);
    if (rc) return rc;
    if (S < 1) return fail(h, PF_EINVAL, "a taxon table needs S >= 1 sets (got %d)", S);
    if (M < 2) return fail(h, PF_EINVAL, "a taxon set needs M >= 2 rows (got %d)", M);
    return check_taxon_sets(h, B, L, S, M, ntab);
}

// whole sources per sub-call: together they hold at most "sub_floats" distances; one source always runs whole
int sub_sources(const pf_handle* h, int B, size_t per_source) {
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)B, (size_t)h->sub_floats / per_source));
}

// The one driver of the host entry points that cut the taxon axis (pf_forward_taxa, pf_forward_leave_one_out,
// pf_forward_place, pf_forward_tiled); the caller has checked its arguments and the residues.
// upload() makes the B sources [N][L] resident in h->d_idx and the caller's row table in h->d_map, once per call: nothing
// that writes h->d_idx (pf_forward's host path) may run after it.  cut() forwards sets of table rows of the current
// sources: all B, until sub_calls() narrows them to one sub-call [b0, b0 + nb) at a time and drains the stream after each.
// There carve() hands out the grow-only h->d_sub as consecutive spans, up() fills one from a host array of the sub-call
// and down() returns one to the batch's host array at b0 * stride.
struct TaxonCuts {
    pf_handle* h;
    int B, N, L;
    int b0 = 0, nb = B;

    int upload(const uint8_t* idx, const int32_t* table, size_t table_bytes) {
        const size_t nidx = (size_t)B * N * L;
        HIPCHK(h, hipSetDevice(h->device));
        int rc = h->d_idx.reserve(h, nidx);
        if (rc || (rc = h->d_map.reserve(h, table_bytes))) return rc;
        HIPCHK(h, hipMemcpyAsync(h->d_idx, idx, nidx, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->d_map, table, table_bytes, hipMemcpyHostToDevice, h->stream));
        return PF_OK;
    }
    // The S sets of M rows each from entry t_off of the table, cut from every current source and forwarded on the path
    // of (M, L), range re-check included, into host dst [nb][S][P_M].  reduce: a reduction will read them from h->d_out,
    // so what the re-check replaced on the host goes up again first - the one place that rule is written.
    int cut(size_t t_off, int S, int M, const char* what, float* dst, bool reduce = false) {
        const int64_t before = h->rechecked;
        const int32_t* d_rows = h->d_map + t_off;
        const int rc = forward_derived(h, nullptr, nb, N, L, S, M, L, dst, what,
                                       [this, d_rows, M](const uint8_t* d_src, int nbc, int j0, int nj, uint8_t* d_dst) -> int {
                                           return launch_gather_taxa(h, d_src, nbc, N, L, d_rows, j0, nj, M, d_dst);
                                       }, nullptr, h->d_idx + (size_t)b0 * N * L);
        return !rc && reduce && h->rechecked != before ? up(h->d_out, dst, (size_t)S * M * (M - 1) / 2) : rc;
    }
    int carve(std::initializer_list<pfspan::FloatSpan> spans) {          // {pointer, floats for every current source}
        auto list = [&](auto& v) { pfspan::float_spans(v, spans, (size_t)nb); };
        if (const int rc = h->d_sub.reserve(h, pfspan::measure(list))) return rc;
        pfspan::carve(h->d_sub, list);
        return PF_OK;
    }
    int copy(float* dst, const float* src, size_t stride, hipMemcpyKind kind) {         // the current sources' floats
        HIPCHK(h, hipMemcpyAsync(dst, src, (size_t)nb * stride * sizeof(float), kind, h->stream));
        return PF_OK;
    }
    float* part(float* host, size_t stride) const { return host + (size_t)b0 * stride; }
    int up(float* d, const float* host_sub, size_t stride) { return copy(d, host_sub, stride, hipMemcpyHostToDevice); }
    int down(float* host, const float* d, size_t stride) { return copy(part(host, stride), d, stride, hipMemcpyDeviceToHost); }
    template <class Body>
    int sub_calls(size_t per_source, Body&& body) {
        const int sub = sub_sources(h, B, per_source);
        for (b0 = 0; b0 < B; b0 += sub) {
            nb = std::min(sub, B - b0);
            if (const int rc = body()) return rc;
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
        return PF_OK;
    }
};

int taxa_impl(pf_handle* h, const uint8_t* idx, int B, int N, int L, const int32_t* taxa, int S, int M, float* out) {
    size_t ntab = 0;
    int rc = check_taxa_call(h, B, N, L, S, M, &ntab);
    if (rc) return rc;
    if (!out || !idx || !taxa) return fail(h, PF_EINVAL, "null buffer");
    const int64_t at = pftaxa::first_bad_taxon(taxa, (size_t)S * M, N);
    if (at >= 0)
        return fail(h, PF_EINVAL, "taxon %d at set %lld, position %lld is outside [0, %d)", (int)taxa[at], (long long)(at / M),
                    (long long)(at % M), N);
    if ((rc = check_residues(h, idx, (size_t)B * N * L))) return rc;
    TaxonCuts c{h, B, N, L};
    if ((rc = c.upload(idx, taxa, ntab))) return rc;
    return c.cut(0, S, M, "taxon sets", out);
}

// pf_forward_leave_one_out: pf_forward of the B sources - before the driver's upload, since its range re-check stages
// into h->d_idx - then their N cuts each (row t of the table: 0 .. N - 1 without t) in sub-calls, each reduced on the
// device from the cuts in h->d_out.
int loo_impl(pf_handle* h, const uint8_t* idx, int B, int N, int L, float* out, float* loo, float* influence, float* shift,
             float* context) {
    int rc = check_dims(h, B, N, L, L);
    if (rc) return rc;
    if (N < 3) return fail(h, PF_EINVAL, "leave-one-out needs N >= 3 sequences (got %d): a cut keeps at least one pair", N);
    size_t ntab = 0;
    if ((rc = check_taxa_call(h, B, N, L, N, N - 1, &ntab))) return rc;
    if (!out || !idx || !influence || !shift || !context) return fail(h, PF_EINVAL, "null buffer");
    if ((rc = check_residues(h, idx, (size_t)B * N * L))) return rc;
    const size_t P = (size_t)N * (N - 1) / 2, P1 = (size_t)(N - 1) * (N - 2) / 2, per_loo = (size_t)N * P1;
    std::vector<int32_t> table;
    std::vector<float> tmp;
    try {
        table.resize((size_t)N * (N - 1));
        if (!loo) tmp.resize((size_t)sub_sources(h, B, per_loo) * per_loo);
    } catch (const std::bad_alloc&) { return fail(h, PF_ENOMEM, "out of host memory for the leave-one-out sets of %d sequences", N); }
    for (int t = 0; t < N; ++t)
        for (int m = 0; m < N - 1; ++m) table[(size_t)t * (N - 1) + m] = m + (m >= t ? 1 : 0);
    if ((rc = forward_host_impl(h, idx, B, N, 0, L, L, out))) return rc;
    TaxonCuts c{h, B, N, L};
    if ((rc = c.upload(idx, table.data(), ntab))) return rc;
    return c.sub_calls(per_loo, [&]() -> int {
        int rc2 = c.cut(0, N, N - 1, "taxon sets", loo ? c.part(loo, per_loo) : tmp.data(), true);
        if (rc2) return rc2;
        float *d_full, *d_ctx, *d_infl, *d_shift;
        if ((rc2 = c.carve({{&d_full, P}, {&d_ctx, P}, {&d_infl, (size_t)N}, {&d_shift, (size_t)N}}))) return rc2;
        if ((rc2 = c.up(d_full, c.part(out, P), P))) return rc2;
        if ((rc2 = launch_loo_stats(h, d_full, h->d_out, c.nb, N, d_infl, d_shift, d_ctx))) return rc2;
        if ((rc2 = c.down(context, d_ctx, P)) || (rc2 = c.down(influence, d_infl, N))) return rc2;
        return c.down(shift, d_shift, N);
    });
}

// ---- query placement (pf_forward_place, pf_place_stats_device; pf_place.hip.h) ---------------

int launch_place_stats(pf_handle* h, const float* d_whole, const float* d_base, const float* d_sets, int B, int N, int Q,
                       float* d_place, float* d_disturb, float* d_shift, float* d_joint) {
    return launch_on_stream(h, K_PLACE_STATS, "k_place_rows / k_place_backbone", [&] {
        return pfpl::launch_place_stats(h->stream, d_whole, d_base, d_sets, B, N, Q, d_place, d_disturb, d_shift, d_joint);
    });
}

// pf_forward_place: three kinds of derived alignments are cut from the resident sources [M][L] - the whole (rows
// 0 .. M - 1: pf_forward's bits, and the resident bytes stay intact where pf_forward's own re-check would stage over
// them), the backbone (rows 0 .. N - 1) and the Q sets (rows 0 .. N - 1, N + q) - each on the path of its own shape.
// Their row tables share one upload: [Q][N + 1], then [N], then [M].  The sets run in sub-calls, each reduced on the
// device from the sets in h->d_out.
int place_impl(pf_handle* h, const uint8_t* idx, int B, int M, int L, int Q, float* out, float* base, float* sets, float* place,
               float* disturb, float* shift, float* joint) {
    int rc = check_dims(h, B, M, L, L);
    if (rc) return rc;
    if (Q < 1) return fail(h, PF_EINVAL, "placement needs Q >= 1 queries (got %d)", Q);
    if (M - Q < 2) return fail(h, PF_EINVAL, "placement needs a backbone of M - Q >= 2 sequences (got M=%d, Q=%d)", M, Q);
    const int N = M - Q;
    size_t n = 0;
    if ((rc = check_taxon_sets(h, B, L, Q, N + 1, &n))) return rc;              // the Q sets of N + 1 rows
    if ((rc = check_dims(h, B, N, L, L))) return rc;
    const size_t PM = (size_t)M * (M - 1) / 2, PN = (size_t)N * (N - 1) / 2, P1 = (size_t)(N + 1) * N / 2;
    if (!mul_size((size_t)B, PM, sizeof(float), &n) || !mul_size((size_t)B, (size_t)M, (size_t)L, &n))
        return fail(h, PF_EINVAL, "B=%d alignments of %d x %d overflow the address space", B, M, L);
    if (!out || !idx || !base || !place || !disturb || !shift || !joint) return fail(h, PF_EINVAL, "null buffer");
    const size_t per_set = (size_t)Q * P1, nplace = (size_t)Q * N, nq = (size_t)Q;
    if ((rc = check_residues(h, idx, (size_t)B * M * L))) return rc;
    const size_t t_base = (size_t)Q * (N + 1), t_whole = t_base + N;
    std::vector<int32_t> table;
    std::vector<float> tmp;
    try {
        table.resize(t_whole + M);
        if (!sets) tmp.resize((size_t)sub_sources(h, B, per_set) * per_set);
    } catch (const std::bad_alloc&) { return fail(h, PF_ENOMEM, "out of host memory for the sets of %d queries", Q); }
    for (int q = 0; q < Q; ++q) {
        for (int m = 0; m < N; ++m) table[(size_t)q * (N + 1) + m] = m;
        table[(size_t)q * (N + 1) + N] = N + q;
    }
    for (int m = 0; m < N; ++m) table[t_base + m] = m;
    for (int m = 0; m < M; ++m) table[t_whole + m] = m;
    TaxonCuts c{h, B, M, L};
    if ((rc = c.upload(idx, table.data(), table.size() * sizeof(int32_t)))) return rc;
    if ((rc = c.cut(t_whole, 1, M, "alignments", out))) return rc;
    if ((rc = c.cut(t_base, 1, N, "backbones", base))) return rc;
    return c.sub_calls(per_set, [&]() -> int {
        int rc2 = c.cut(0, Q, N + 1, "query sets", sets ? c.part(sets, per_set) : tmp.data(), true);
        if (rc2) return rc2;
        float *d_whole, *d_base, *d_pl, *d_dis, *d_sh, *d_jt;
        if ((rc2 = c.carve({{&d_whole, PM}, {&d_base, PN}, {&d_pl, nplace}, {&d_dis, nq}, {&d_sh, nq}, {&d_jt, nq}}))) return rc2;
        if ((rc2 = c.up(d_whole, c.part(out, PM), PM)) || (rc2 = c.up(d_base, c.part(base, PN), PN))) return rc2;
        if ((rc2 = launch_place_stats(h, d_whole, d_base, h->d_out, c.nb, N, Q, d_pl, d_dis, d_sh, d_jt))) return rc2;
        if ((rc2 = c.down(place, d_pl, nplace)) || (rc2 = c.down(disturb, d_dis, nq)) || (rc2 = c.down(shift, d_sh, nq))) return rc2;
        return c.down(joint, d_jt, nq);
    });
}

// ---- tiled inference (pf_forward_tiled, pf_tile_combine_device; pf_tile.hip.h, pf_tile_host.h) ----

// The plan of (N, M) in h->tiled_plan and its two tables on the device (h->tiled_tab),
// rebuilt only when (N, M) changes.  The stream is drained first: the upload of the previous tables may still be reading
// the host vectors.  The caller has checked M >= 2 and N > M.
int ensure_tiled_plan(pf_handle* h, int N, int M) {
    pftile::Plan& p = h->tiled_plan;
    if (p.N == N && p.M == M && h->d_tiled_tab) return PF_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    bool ok = false;
    try { ok = p.build(N, M); } catch (const std::bad_alloc&) {
        p.N = p.M = 0;
        return fail(h, PF_ENOMEM, "out of host memory for the tiling plan of N=%d, M=%d", N, M);
    }
    if (!ok) return fail(h, PF_EINVAL, "tiling needs 2 <= M < N (got N=%d, M=%d)", N, M);
    pftile::Tables& t = h->tiled_tab;
    auto list = [&](auto& v) { pftile::table_arrays(v, t, p); };
    int rc = h->d_tiled_tab.reserve(h, pfspan::measure(list));
    hipError_t e = hipSuccess;
    if (!rc) {
        pfspan::carve(h->d_tiled_tab, list);
        e = hipMemcpyAsync(t.offset, p.offset.data(), p.offset.size() * sizeof(int64_t), hipMemcpyHostToDevice, h->stream);
    }
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(t.bounds, p.bounds.data(), p.bounds.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream);
    if (rc || e != hipSuccess) {
        p.N = p.M = 0;                                   // (the tables on the device are not this plan's)
        return rc ? rc : fail(h, PF_EHIP, "upload of the tiling plan failed: %s", hipGetErrorString(e));
    }
    return PF_OK;
}

// d_sets [B][T] -> d_out, d_spread [B][P_N] by the resident plan
int launch_tile_combine(pf_handle* h, const float* d_sets, int B, float* d_out, float* d_spread) {
    const pftile::Plan& p = h->tiled_plan;
    return launch_on_stream(h, K_TILE_COMBINE, "k_tile_combine", [&] {
        return pftile::launch_tile_combine(h->stream, d_sets, h->tiled_tab.bounds, h->tiled_tab.offset, B, p.N, p.G, p.T, d_out, d_spread);
    });
}

// What pf_forward_tiled and pf_tile_combine_device refuse about (B, N, M) beside the handle's own state: the context, the
// cap - against M, never against N - and the sizes.
int check_tiled_shape(pf_handle* h, int B, int N, int M) {
    if (M < 2) return fail(h, PF_EINVAL, "tiling needs a context of M >= 2 sequences (got %d)", M);
    if (B < 1) return fail(h, PF_EINVAL, "bad dimensions B=%d N=%d M=%d", B, N, M);
    if (h->max_seqs > 0 && M > h->max_seqs)
        // (pf_forward's wording: the context is what a forward sees)
        return fail(h, PF_EINVAL, "n_seqs must be smaller or equal to %lld (or pre-compute a larger global_seq2pair)",
                    (long long)h->max_seqs);
    if (M > 32767) return fail(h, PF_EINVAL, "n_seqs %d exceeds the pair-table index range", M);
    if (N <= M) return fail(h, PF_EINVAL, "N=%d sequences fit one context of M=%d: call pf_forward", N, M);
    const int64_t PN = (int64_t)N * (N - 1) / 2;
    size_t n = 0;
    if (PN >= ((int64_t)1 << 31) || !mul_size((size_t)B, (size_t)PN, 2 * sizeof(float), &n))
        return fail(h, PF_EINVAL, "B=%d alignments of N=%d sequences: their %lld pairs each overflow a distance vector", B, N, (long long)PN);
    return PF_OK;
}

// pf_forward_tiled: the sets of one size - a class, at most three - share a row table [S_c][m_c]; the tables go up
// together, and every class is one cut, so that every set takes pf_forward's path for (m_c, L), range re-check included.
// The class results are assembled on the host into the [nb][T] layout of k_tile_combine - after the re-check has
// replaced flagged sets - uploaded once and combined on the device, T distances per source to a sub-call.  Nothing is
// written to out / spread before the first sub-call has succeeded.
int tiled_impl(pf_handle* h, const uint8_t* idx, int B, int N, int L, int M, float* out, float* spread) {
    int rc = check_tiled_shape(h, B, N, M);
    if (rc) return rc;
    if ((rc = check_dims(h, B, M, L, L))) return rc;                           // the handle's weights, L
    if (h->world > 1)
        return fail(h, PF_ESTATE, "tiled inference is not site-sharded: this handle's communicator has %d ranks (use a handle "
                                  "without a communicator)", h->world);
    size_t nidx = 0;
    if (!mul_size((size_t)B, (size_t)N, (size_t)L, &nidx))
        return fail(h, PF_EINVAL, "B=%d alignments of %d x %d overflow the address space", B, N, L);
    if (!out || !spread || !idx) return fail(h, PF_EINVAL, "null buffer");
    if ((rc = check_residues(h, idx, nidx))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = ensure_tiled_plan(h, N, M))) return rc;
    const pftile::Plan& p = h->tiled_plan;
    const size_t T = (size_t)p.T, PN = (size_t)N * (N - 1) / 2;
    const int sub = sub_sources(h, B, T);
    size_t t_off[3] = {0, 0, 0}, pairs[3] = {0, 0, 0}, ntab = 0, ncls = 0, n = 0;
    for (int c = 0; c < p.n_class; ++c) {
        const int m = p.class_m[c];
        if ((rc = check_dims(h, sub, m, L, L))) return rc;                     // every set size against "max_seqs"
        pairs[c] = (size_t)m * (m - 1) / 2;
        if (p.class_sets[c] > INT32_MAX || !mul_size((size_t)sub, (size_t)p.class_sets[c], pairs[c] * sizeof(float), &n) ||
            !mul_size((size_t)sub, (size_t)p.class_sets[c], (size_t)m * L, &n))
            return fail(h, PF_EINVAL, "%lld tile sets of %d x %d overflow the address space", (long long)p.class_sets[c], m, L);
        t_off[c] = ntab;
        ntab += (size_t)p.class_sets[c] * m;
        ncls = std::max(ncls, (size_t)sub * (size_t)p.class_sets[c] * pairs[c]);
    }
    std::vector<int32_t> table;
    std::vector<int64_t> members[3];           // the sets of every class, in (g, h) order
    std::vector<float> cls, staged;
    try {
        table.resize(ntab);
        for (int c = 0; c < p.n_class; ++c) members[c].reserve((size_t)p.class_sets[c]);
        cls.resize(ncls);
        staged.resize((size_t)sub * T);
    } catch (const std::bad_alloc&) { return fail(h, PF_ENOMEM, "out of host memory for the %lld tile sets of N=%d, M=%d", (long long)p.S, N, M); }
    int64_t k = 0;
    for (int g = 0; g < p.G; ++g)
        for (int g2 = g + 1; g2 < p.G; ++g2, ++k) {
            const int c = p.class_of(p.rows(g) + p.rows(g2));
            int32_t* row = table.data() + t_off[c] + members[c].size() * (size_t)p.class_m[c];
            for (int r = p.bounds[g]; r < p.bounds[g + 1]; ++r) *row++ = r;
            for (int r = p.bounds[g2]; r < p.bounds[g2 + 1]; ++r) *row++ = r;
            members[c].push_back(k);
        }
    TaxonCuts c{h, B, N, L};
    if ((rc = c.upload(idx, table.data(), ntab * sizeof(int32_t)))) return rc;
    return c.sub_calls(T, [&]() -> int {
        for (int cl = 0; cl < p.n_class; ++cl) {
            const int Sc = (int)p.class_sets[cl];
            const int rc2 = c.cut(t_off[cl], Sc, p.class_m[cl], "tile sets", cls.data());
            if (rc2) return rc2;
            for (int b = 0; b < c.nb; ++b)
                for (int j = 0; j < Sc; ++j)
                    memcpy(staged.data() + (size_t)b * T + (size_t)p.offset[(size_t)members[cl][(size_t)j]],
                           cls.data() + ((size_t)b * Sc + j) * pairs[cl], pairs[cl] * sizeof(float));
        }
        float *d_sets, *d_o, *d_sp;
        int rc2 = c.carve({{&d_sets, T}, {&d_o, PN}, {&d_sp, PN}});
        if (rc2 || (rc2 = c.up(d_sets, staged.data(), T))) return rc2;
        if ((rc2 = launch_tile_combine(h, d_sets, c.nb, d_o, d_sp))) return rc2;
        if ((rc2 = c.down(out, d_o, PN))) return rc2;
        return c.down(spread, d_sp, PN);
    });
}

// ---- neighbour joining on the device (pf_nj_joins, pf_nj_joins_device; pf_nj.hip.h, pf_nj_host.h) ----

// A tree search as its entry points' check sees it: its name, its largest N (0: none), the bytes of its state per
// source, the sources of one launch, and what the refusal says the state holds.
struct TreeSearch { const char* what; int max_n; size_t (*state_bytes)(int); int max_sources; const char* holds; };
const TreeSearch NJ_SEARCH{"neighbour joining", 0, pfnj::state_bytes, pfnj::NJ_MAX_Y, "N^2 doubles"};
const TreeSearch BIONJ_SEARCH{"BIONJ", 0, pfbionj::state_bytes, pfbionj::BIONJ_MAX_Y, "2 N^2 doubles"};
const TreeSearch NNI_SEARCH{"balanced NNI", pfbme::MAX_N, pfbme::state_bytes, pfbme::BME_MAX_Z, "its table of 4N-6 subtrees"};
const TreeSearch SPR_SEARCH{"balanced SPR", pfbme::MAX_N, pfbme::spr_state_bytes, pfbme::BME_MAX_Z,
                            "its table of 4N-6 subtrees and their pair table"};

// What the entry points of a tree search refuse about (B, N), and the sources of one chunk: as many as fit
// "ws_limit_mb" side by side, one at least - a single source's state above the limit is refused.
int check_tree_shape(pf_handle* h, const TreeSearch& t, int B, int N, int* chunk) {
    if (B < 1) return fail(h, PF_EINVAL, "bad dimensions B=%d N=%d", B, N);
    if (N < 3) return fail(h, PF_EINVAL, "%s needs N >= 3 sequences (got %d)", t.what, N);
    if (t.max_n && N > t.max_n) return fail(h, PF_EINVAL, "%s takes at most %d sequences (got %d)", t.what, t.max_n, N);
    const int64_t PN = (int64_t)N * (N - 1) / 2;
    size_t n = 0;
    if (PN >= ((int64_t)1 << 31) || !mul_size((size_t)B, (size_t)PN, sizeof(float), &n) ||
        !mul_size((size_t)B, (size_t)pfnj::table_len(N), sizeof(double), &n))
        return fail(h, PF_EINVAL, "B=%d alignments of N=%d sequences: their %lld pairs each overflow a distance vector", B, N, (long long)PN);
    const size_t per = t.state_bytes(N);
    if ((int64_t)per > h->ws_limit_bytes)
        return fail(h, PF_EINVAL, "%s of N=%d sequences needs %zu bytes of state per source (%s), above the workspace limit of %lld bytes "
                                  "(option ws_limit_mb)", t.what, N, per, t.holds, (long long)h->ws_limit_bytes);
    *chunk = (int)std::min<size_t>(std::min(B, t.max_sources), (size_t)h->ws_limit_bytes / per);
    return PF_OK;
}

// ---- a host entry point on staged arrays.  The list of a call's arrays (pf_spans.h) names each
// with its staging pointer, the caller's, its elements, its direction and what a null means: nothing here repeats them.

// the list's inputs to their staging (`up`) or its results to the caller, by hipMemcpyAsync on h->stream
template <class List>
int list_copy(pf_handle* h, List&& list, bool up, hipMemcpyKind kind) {
    auto copy = [&](void* to, const void* from, size_t bytes) { return hipMemcpyAsync(to, from, bytes, kind, h->stream); };
    const hipError_t e = (hipError_t)(up ? pfspan::upload(list, copy) : pfspan::download(list, copy));
    if (e != hipSuccess)
        return fail(h, e == hipErrorOutOfMemory ? PF_ENOMEM : PF_EHIP, "hipMemcpyAsync of a call's %s: %s", up ? "inputs" : "results",
                    hipGetErrorString(e));
    return PF_OK;
}

// The call: the list's arrays carved from `buf`, the inputs up, launch() - which reads the staging pointers the list
// has set -, the results down, one synchronisation.
template <class List, class Launch>
int staged_call(pf_handle* h, Buffer<char>& buf, List&& list, Launch&& launch) {
    int rc = buf.reserve(h, pfspan::measure(list));
    if (rc) return rc;
    pfspan::carve(buf, list);
    if ((rc = list_copy(h, list, true, hipMemcpyHostToDevice)) || (rc = launch()) || (rc = list_copy(h, list, false, hipMemcpyDeviceToHost)))
        return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PF_OK;
}

// the join sequences of nb <= chunk sources on device arrays, enqueued on h->stream: neighbour joining, or BIONJ
// (pf_bionj.hip.h)
int launch_nj_chunk(pf_handle* h, bool bionj, const pfnj::Tables& d, int nb, int N) {
    const int rc = h->d_nj.reserve(h, (size_t)nb * (bionj ? pfbionj::state_bytes(N) : pfnj::state_bytes(N)));
    if (rc) return rc;
    h->cur = h->stream;
    const hipError_t e = bionj ? pfbionj::launch_bionj(h->stream, pfbionj::carve(h->d_nj, d.preds, nb, N, d.slots, d.lengths, d.flag), nb)
                               : pfnj::launch_nj(h->stream, pfnj::carve(h->d_nj, d.preds, nb, N, d.slots, d.lengths, d.flag), nb);
    if (e != hipSuccess) return fail(h, PF_EHIP, "%s launch failed: %s", bionj ? "k_bionj_*" : "k_nj_*", hipGetErrorString(e));
    return PF_OK;
}

// The caller's arrays on the device (asynchronous) or on the host: then every chunk is staged, and synchronises once.
int nj_impl(pf_handle* h, bool bionj, bool device, const pfnj::Tables& user, int B, int N) {
    pfnj::Tables io{};
    auto chunk_list = [&](int b0, int nb) {
        return [&io, N, nb, u = pfnj::chunk_of(user, (size_t)b0, N)](auto& v) { pfnj::staging_arrays(v, io, u, (size_t)nb, N); };
    };
    if (pfspan::missing(chunk_list(0, 0))) return fail(h, PF_EINVAL, "null buffer");
    int chunk = 0;
    int rc = check_tree_shape(h, bionj ? BIONJ_SEARCH : NJ_SEARCH, B, N, &chunk);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    ++(bionj ? h->bionj_calls : h->nj_calls);
    // (a flagged source's table is unspecified, not uninitialised: the staged tables are zeroed, the flags always written)
    auto zero = [&](void*, void* staged, size_t bytes) { return staged == io.flag ? hipSuccess : hipMemsetAsync(staged, 0, bytes, h->stream); };
    // (chunks follow each other on the stream, so the next one reuses the state launch_nj_chunk reserved for the first,
    // and the staging the first - the largest - reserved)
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        if (device) rc = launch_nj_chunk(h, bionj, pfnj::chunk_of(user, (size_t)b0, N), nb, N);
        else rc = staged_call(h, h->d_nj_io, chunk_list(b0, nb), [&]() -> int {
            HIPCHK(h, (hipError_t)pfspan::download(chunk_list(b0, nb), zero));
            return launch_nj_chunk(h, bionj, io, nb, N);
        });
        if (rc) return rc;
    }
    return PF_OK;
}

// ---- delta scores on the device (pf_delta, pf_delta_device; pf_delta.hip.h, pf_delta_host.h) ----

// The caller's arrays on the device (asynchronous) or on the host (staged, one synchronisation).  The kernels keep no
// state per source, so a call is not cut into chunks of sources: its launches are cut by their work (launch_delta).
int delta_impl(pf_handle* h, bool device, const pfdelta::Tables& user, int B, int N, int K) {
    pfdelta::Tables io{};
    auto list = [&](auto& v) { pfdelta::staging_arrays(v, io, user, (size_t)std::max(B, 0), std::max(N, 0), std::max(K, 0)); };
    if (pfspan::missing(list)) return fail(h, PF_EINVAL, "null buffer");
    switch (pfdelta::refused(B, N, K)) {
        case 1: return fail(h, PF_EINVAL, "delta scores take %d <= N <= %d sequences (got %d)", pfdelta::MIN_N, pfdelta::MAX_N, N);
        case 2: return fail(h, PF_EINVAL, "bad dimensions B=%d N=%d", B, N);
        case 3: return fail(h, PF_EINVAL, "delta scores take 1 <= K <= %d bins (got %d)", pfdelta::MAX_K, K);
    }
    size_t n = 0;
    if (!mul_size((size_t)B, (size_t)N * (size_t)(N - 1) / 2, sizeof(int64_t), &n))
        return fail(h, PF_EINVAL, "B=%d sources of N=%d sequences overflow the address space", B, N);
    HIPCHK(h, hipSetDevice(h->device));
    ++h->delta_calls;
    auto launch = [&](const pfdelta::Tables& d) -> int {
        h->cur = h->stream;
        const hipError_t e = pfdelta::launch_delta(h->stream, d.preds, B, N, K, d.pair_sum, d.hist, d.flag, h->delta_atomic);
        if (e != hipSuccess) return fail(h, PF_EHIP, "k_delta_* launch failed: %s", hipGetErrorString(e));
        return PF_OK;
    };
    if (device) return launch(user);
    return staged_call(h, h->d_delta_io, list, [&] { return launch(io); });
}

// ---- tree fit on the device (pf_tree_fit, pf_tree_fit_device; pf_fit.hip.h, pf_fit_host.h) ----

// The caller's arrays on the device (asynchronous) or on the host (staged, one synchronisation).  The items - the B M
// trees - are cut into chunks whose node arrays (and, where the caller keeps no patristic, whose distances) fit
// "ws_limit_mb" side by side; the chunks follow each other on the stream and reuse the workspace.
int fit_impl(pf_handle* h, bool device, const pffit::Tables& user, int B, int M, int N) {
    pffit::Tables io{};
    auto list = [&](auto& v) { pffit::staging_arrays(v, io, user, (size_t)std::max(B, 0), (size_t)std::max(M, 0), N); };
    if (pfspan::missing(list)) return fail(h, PF_EINVAL, "null buffer");
    switch (pffit::refused(B, M, N)) {
        case 1: return fail(h, PF_EINVAL, "tree fit needs N >= %d sequences (got %d)", pffit::MIN_N, N);
        case 2: return fail(h, PF_EINVAL, "tree fit takes at most %d sequences (got %d)", pffit::MAX_N, N);
        case 3: return fail(h, PF_EINVAL, "tree fit needs B >= 1 sources (got %d)", B);
        case 4: return fail(h, PF_EINVAL, "tree fit needs M >= 1 trees per source (got %d)", M);
        case 5: return fail(h, PF_EINVAL, "N=%d sequences have 2^31 pairs or more", N);
    }
    const int64_t P = (int64_t)N * (N - 1) / 2, items = (int64_t)B * M;
    size_t n = 0;
    if (!mul_size((size_t)items, (size_t)P, sizeof(double), &n) || !mul_size((size_t)items, (size_t)N, pffit::COLS * sizeof(double), &n))
        return fail(h, PF_EINVAL, "B=%d sources of M=%d trees of N=%d sequences overflow the address space", B, M, N);
    const size_t per = pffit::state_bytes(N, !user.patristic);
    if ((int64_t)per > h->ws_limit_bytes)
        return fail(h, PF_EINVAL, "tree fit of N=%d sequences needs %zu bytes of state per tree (its node arrays%s), above the workspace "
                                  "limit of %lld bytes (option ws_limit_mb)", N, per, user.patristic ? "" : " and its distances",
                    (long long)h->ws_limit_bytes);
    const int chunk = (int)std::min<int64_t>(std::min(items, pffit::max_items(N)), (int64_t)((size_t)h->ws_limit_bytes / per));
    HIPCHK(h, hipSetDevice(h->device));
    ++h->fit_calls;
    auto launch = [&](const pffit::Tables& d) -> int {
        const int rc = h->d_fit.reserve(h, (size_t)chunk * per);
        if (rc) return rc;
        h->cur = h->stream;
        // (a tree with a status is walked by no kernel: its results are these zeros)
        if (d.patristic) HIPCHK(h, hipMemsetAsync(d.patristic, 0, (size_t)items * (size_t)P * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(d.rows, 0, (size_t)items * (size_t)N * pffit::COLS * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(d.worst_j, 0, (size_t)items * (size_t)N * sizeof(int32_t), h->stream));
        pffit::Args a{};
        a.preds = d.preds; a.slots = d.slots; a.lengths = d.lengths;
        a.rows = d.rows; a.worst_j = d.worst_j; a.status = d.status;
        a.P = P; a.N = N; a.M = M;
        for (int64_t item0 = 0; item0 < items; item0 += chunk) {
            a.item0 = item0; a.nb = (int)std::min<int64_t>(chunk, items - item0);
            pffit::carve(a, h->d_fit, a.nb, !d.patristic);
            if (d.patristic) a.tree = d.patristic + (size_t)item0 * (size_t)P;
            const hipError_t e = pffit::launch_chunk(h->stream, a, (int)h->fit_lds_bytes);
            if (e != hipSuccess) return fail(h, PF_EHIP, "k_fit_* launch failed: %s", hipGetErrorString(e));
        }
        return PF_OK;
    };
    if (device) return launch(user);
    return staged_call(h, h->d_fit_io, list, [&] { return launch(io); });
}

// ---- least-squares branch lengths on the device (pf_tree_ols, pf_tree_ols_device; pf_ols.hip.h, pf_ols_host.h) ----

// The caller's arrays on the device (asynchronous) or on the host (staged, one synchronisation).  The items - the B M
// trees - are cut into chunks whose column sums and node arrays fit "ws_limit_mb" side by side; the chunks follow each
// other on the stream and reuse the workspace.
int ols_impl(pf_handle* h, bool device, const pfols::Tables& user, int B, int M, int N) {
    pfols::Tables io{};
    auto list = [&](auto& v) { pfols::staging_arrays(v, io, user, (size_t)std::max(B, 0), (size_t)std::max(M, 0), N); };
    if (pfspan::missing(list)) return fail(h, PF_EINVAL, "null buffer");
    switch (pfols::refused(B, M, N)) {
        case 1: return fail(h, PF_EINVAL, "tree OLS needs N >= %d sequences (got %d)", pfols::MIN_N, N);
        case 2: return fail(h, PF_EINVAL, "tree OLS takes at most %d sequences (got %d)", pfols::MAX_N, N);
        case 3: return fail(h, PF_EINVAL, "tree OLS needs B >= 1 sources (got %d)", B);
        case 4: return fail(h, PF_EINVAL, "tree OLS needs M >= 1 trees per source (got %d)", M);
    }
    const int64_t P = (int64_t)N * (N - 1) / 2, items = (int64_t)B * M;
    const int T = pfols::table_len(N);
    size_t n = 0;
    if (!mul_size((size_t)items, (size_t)T, sizeof(double), &n) || !mul_size((size_t)B, (size_t)P, sizeof(float), &n))
        return fail(h, PF_EINVAL, "B=%d sources of M=%d trees of N=%d sequences overflow the address space", B, M, N);
    const size_t per = pfols::state_bytes(N);
    if ((int64_t)per > h->ws_limit_bytes)
        return fail(h, PF_EINVAL, "tree OLS of N=%d sequences needs %zu bytes of state per tree (its column sums and node arrays), above "
                                  "the workspace limit of %lld bytes (option ws_limit_mb)", N, per, (long long)h->ws_limit_bytes);
    const int chunk = (int)std::min<int64_t>(std::min(items, pfols::max_items(N)), (int64_t)((size_t)h->ws_limit_bytes / per));
    HIPCHK(h, hipSetDevice(h->device));
    ++h->ols_calls;
    auto launch = [&](const pfols::Tables& d) -> int {
        const int rc = h->d_ols.reserve(h, (size_t)chunk * per);
        if (rc) return rc;
        h->cur = h->stream;
        // (a tree with a status is walked by no kernel: its results are these zeros)
        HIPCHK(h, hipMemsetAsync(d.ols, 0, (size_t)items * (size_t)T * sizeof(double), h->stream));
        pfols::Args a{};
        a.preds = d.preds; a.slots = d.slots; a.ols = d.ols; a.status = d.status;
        a.P = P; a.N = N; a.M = M;
        for (int64_t item0 = 0; item0 < items; item0 += chunk) {
            a.item0 = item0; a.nb = (int)std::min<int64_t>(chunk, items - item0);
            pfols::carve(a, h->d_ols, a.nb);
            const hipError_t e = pfols::launch_chunk(h->stream, a);
            if (e != hipSuccess) return fail(h, PF_EHIP, "k_ols_* launch failed: %s", hipGetErrorString(e));
        }
        return PF_OK;
    };
    if (device) return launch(user);
    return staged_call(h, h->d_ols_io, list, [&] { return launch(io); });
}

// ---- tree rooting on the device (pf_tree_root, pf_tree_root_device; pf_root.hip.h, pf_root_host.h) ----

// ols_impl's forms and chunks: the items - the B M trees - are cut into chunks whose path lengths, weights and node arrays
// fit "ws_limit_mb" side by side; the chunks follow each other on the stream and reuse the workspace.
int root_impl(pf_handle* h, bool device, const pfroot::Tables& user, int B, int M, int N) {
    pfroot::Tables io{};
    auto list = [&](auto& v) { pfroot::staging_arrays(v, io, user, (size_t)std::max(B, 0), (size_t)std::max(M, 0), N); };
    if (pfspan::missing(list)) return fail(h, PF_EINVAL, "null buffer");
    switch (pfroot::refused(B, M, N)) {
        case 1: return fail(h, PF_EINVAL, "tree root needs N >= %d sequences (got %d)", pfroot::MIN_N, N);
        case 2: return fail(h, PF_EINVAL, "tree root takes at most %d sequences (got %d)", pfroot::MAX_N, N);
        case 3: return fail(h, PF_EINVAL, "tree root needs B >= 1 sources (got %d)", B);
        case 4: return fail(h, PF_EINVAL, "tree root needs M >= 1 trees per source (got %d)", M);
    }
    const int64_t items = (int64_t)B * M;
    const int T = pfroot::table_len(N);
    size_t n = 0;
    if (!mul_size((size_t)items, (size_t)T, sizeof(double), &n))
        return fail(h, PF_EINVAL, "B=%d sources of M=%d trees of N=%d sequences overflow the address space", B, M, N);
    const size_t per = pfroot::state_bytes(N);
    if ((int64_t)per > h->ws_limit_bytes)
        return fail(h, PF_EINVAL, "tree root of N=%d sequences needs %zu bytes of state per tree (its path lengths, weights and node "
                                  "arrays), above the workspace limit of %lld bytes (option ws_limit_mb)", N, per, (long long)h->ws_limit_bytes);
    const int chunk = (int)std::min<int64_t>(std::min(items, pfroot::max_items(N)), (int64_t)((size_t)h->ws_limit_bytes / per));
    HIPCHK(h, hipSetDevice(h->device));
    ++h->root_calls;
    auto launch = [&](const pfroot::Tables& d) -> int {
        const int rc = h->d_root.reserve(h, (size_t)chunk * per);
        if (rc) return rc;
        h->cur = h->stream;
        // (a tree with a status is walked by no kernel: its results are these zeros)
        HIPCHK(h, hipMemsetAsync(d.ssq, 0, (size_t)items * (size_t)T * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(d.pos, 0, (size_t)items * (size_t)T * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(d.mid, 0, (size_t)items * pfroot::MID * sizeof(double), h->stream));
        pfroot::Args a{};
        a.slots = d.slots; a.lengths = d.lengths; a.ssq = d.ssq; a.pos = d.pos; a.mid = d.mid; a.status = d.status;
        a.N = N;
        for (int64_t item0 = 0; item0 < items; item0 += chunk) {
            a.item0 = item0; a.nb = (int)std::min<int64_t>(chunk, items - item0);
            pfroot::carve(a, h->d_root, a.nb);
            const hipError_t e = pfroot::launch_chunk(h->stream, a);
            if (e != hipSuccess) return fail(h, PF_EHIP, "k_root_* launch failed: %s", hipGetErrorString(e));
        }
        return PF_OK;
    };
    if (device) return launch(user);
    return staged_call(h, h->d_root_io, list, [&] { return launch(io); });
}

// ---- balanced NNI refinement on the device (pf_bme_nni, pf_bme_nni_device; pf_bme.hip.h, pf_bme_host.h) ----

// every start table is a join table (slots in [0, N), every join of two live clusters, three distinct live slots last)
int check_bme_starts(pf_handle* h, const int32_t* start, int B, int N) {
    std::vector<int32_t> parent((size_t)pfbme::nodes_of(N)), children((size_t)pfbme::nodes_of(N) * 3);
    for (int b = 0; b < B; ++b)
        if (!pfbme::tree_of_joins(start + (size_t)b * (size_t)pfnj::table_len(N), N, parent.data(), children.data()))
            return fail(h, PF_EINVAL, "source %d: the start table is not a join table of N=%d sequences", b, N);
    return PF_OK;
}

// The refinement of nb <= chunk sources by balanced NNI or, `spr`, by balanced SPR (DESIGN.md sections 21, 22):
// distances on the device, start tables and results on the host.  Synchronises h->stream once per round of ROUND_STEPS
// steps and once at the end.  The two searches differ at three points: what a round launches; what comes down after it
// (NNI: the trees too; SPR forms its whole table on the device, so the host reads the flags only, and the trees at the
// end); and whether the host rebuilds depth between rounds (NNI).
int bme_chunk(pf_handle* h, bool spr, const float* d_preds, const int32_t* start, int nb, int N, int32_t* slots, double* lengths,
              int32_t* steps, double* tree_length, uint8_t* status) {
    const size_t b = (size_t)nb, T = (size_t)pfnj::table_len(N), nodes = (size_t)pfbme::nodes_of(N), rows = (size_t)pfbme::rows_of(N),
                 root = (size_t)pfbme::root_of(N);
    int rc = h->d_bme.reserve(h, b * (spr ? pfbme::spr_state_bytes(N) : pfbme::state_bytes(N)));
    if (rc) return rc;
    h->cur = h->stream;
    pfbme::SprArgs s{};                                  // (balanced NNI: s.b alone)
    if (spr) s = pfbme::carve_spr(h->d_bme, d_preds, nb, N, h->spr_step_cap);
    else s.b = pfbme::carve(h->d_bme, d_preds, nb, N);
    const pfbme::Args& a = s.b;
    uint8_t* const d_done = spr ? s.sdone : a.done;      // the flag the round's last kernel sets (Args::done stays 0 under SPR)
    std::vector<int32_t> parent(b * nodes), children(b * nodes * 3), nsteps(b, 0), fresh(b, 0);
    std::vector<int16_t> depth(spr ? 0 : b * rows * nodes);
    std::vector<uint8_t> done(b, 0), rebuild(b, 1), st(b, 0);
    std::vector<double> edge_len(b * root);
    for (size_t i = 0; i < b; ++i) {
        pfbme::tree_of_joins(start + i * T, N, &parent[i * nodes], &children[i * nodes * 3]);       // (checked by the caller)
        if (!spr) pfbme::build_depth(&parent[i * nodes], &children[i * nodes * 3], N, &depth[i * rows * nodes]);
    }
    auto up = [&](void* dst, const void* src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream); };
    auto down = [&](void* dst, const void* src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream); };
    HIPCHK(h, up(a.parent, parent.data(), parent.size() * sizeof(int32_t)));
    HIPCHK(h, up(a.children, children.data(), children.size() * sizeof(int32_t)));
    if (!spr) HIPCHK(h, up(a.depth, depth.data(), depth.size() * sizeof(int16_t)));
    HIPCHK(h, up(a.rebuild, rebuild.data(), b));
    HIPCHK(h, hipMemsetAsync(a.steps, 0, b * sizeof(int32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(a.done, 0, b, h->stream));
    HIPCHK(h, hipMemsetAsync(a.status, 0, b, h->stream));
    if (spr) HIPCHK(h, hipMemsetAsync(s.sdone, 0, b, h->stream));
    // (a flagged source's lengths are never written: not uninitialised either)
    HIPCHK(h, hipMemsetAsync(a.edge_len, 0, b * root * sizeof(double), h->stream));
    hipError_t e = pfbme::launch_init(h->stream, a, nb);
    if (e != hipSuccess) return fail(h, PF_EHIP, "k_bme_init launch failed: %s", hipGetErrorString(e));
    for (;;) {
        if (spr) {
            hipEvent_t ev[2] = {};                      // option "profile": the pair table of the round's first step
            if (h->profile && !h->profile_main_only) { ev[0] = get_event(h); ev[1] = get_event(h); }
            e = pfbme::launch_spr_round(h->stream, s, nb, h->spr_pairs_simple, ev[0] ? ev : nullptr);
            if (ev[0]) h->pending.push_back({K_BME_PAIRS, ev[0], ev[1]});
        } else {
            e = pfbme::launch_round(h->stream, a, nb);
        }
        if (e != hipSuccess) return fail(h, PF_EHIP, "k_bme_* launch failed: %s", hipGetErrorString(e));
        HIPCHK(h, down(done.data(), d_done, b));
        HIPCHK(h, down(st.data(), a.status, b));
        if (!spr) {
            HIPCHK(h, down(nsteps.data(), a.steps, b * sizeof(int32_t)));
            HIPCHK(h, down(parent.data(), a.parent, parent.size() * sizeof(int32_t)));
            HIPCHK(h, down(children.data(), a.children, children.size() * sizeof(int32_t)));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (spr) {
            bool all = true;
            for (size_t i = 0; i < b; ++i) all = all && (done[i] || st[i] == pfbme::ST_NONFINITE);
            if (all) break;
            continue;
        }
        if (pfbme::between_rounds(nb, N, parent.data(), children.data(), nsteps.data(), done.data(), st.data(), rebuild.data(), fresh.data(),
                                  depth.data()))
            break;
        HIPCHK(h, up(a.done, done.data(), b));
        HIPCHK(h, up(a.rebuild, rebuild.data(), b));
        for (size_t i = 0; i < b; ++i)
            if (rebuild[i]) HIPCHK(h, up(a.depth + i * rows * nodes, &depth[i * rows * nodes], rows * nodes * sizeof(int16_t)));
    }
    if ((e = spr ? pfbme::launch_spr_finish(h->stream, s, nb) : pfbme::launch_lengths(h->stream, a, nb)) != hipSuccess)
        return fail(h, PF_EHIP, "%s launch failed: %s", spr ? "k_bme_eval / k_bme_lengths" : "k_bme_lengths", hipGetErrorString(e));
    HIPCHK(h, down(edge_len.data(), a.edge_len, edge_len.size() * sizeof(double)));
    if (spr) {
        HIPCHK(h, down(nsteps.data(), a.steps, b * sizeof(int32_t)));
        HIPCHK(h, down(children.data(), a.children, children.size() * sizeof(int32_t)));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < b; ++i)
        pfbme::result_of(N, &children[i * nodes * 3], &edge_len[i * root], nsteps[i], st[i], slots + i * T, lengths + i * T, steps + i,
                         tree_length + i, status + i);
    return PF_OK;
}

// preds and the caller's tables on the host (device = false) or on the device.  spr: the balanced SPR search instead
// of balanced NNI.
int bme_impl(pf_handle* h, bool spr, bool device, const float* preds, const pfbme::Tables& user, int B, int N) {
    // The device form mirrors the caller's six arrays on the host, by the list a host form stages with, in the other
    // direction: the start tables come down before the search, the five results go up after it.
    pfbme::Tables io = user;
    auto list = [&](auto& v) { pfbme::mirror_arrays(v, io, user, (size_t)B, N); };
    if (!preds || pfspan::missing(list)) return fail(h, PF_EINVAL, "null buffer");
    int chunk = 0;
    int rc = check_tree_shape(h, spr ? SPR_SEARCH : NNI_SEARCH, B, N, &chunk);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    try {
        const size_t PN = (size_t)N * (N - 1) / 2, T = (size_t)pfnj::table_len(N);
        pfspan::Allocate own;
        if (device) {
            list(own);
            if ((rc = list_copy(h, list, true, hipMemcpyDeviceToHost))) return rc;
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
        if ((rc = check_bme_starts(h, io.start, B, N))) return rc;
        ++(spr ? h->spr_calls : h->bme_calls);
        if (!device && (rc = h->d_bme_preds.reserve(h, (size_t)chunk * PN * sizeof(float)))) return rc;
        for (int b0 = 0; b0 < B; b0 += chunk) {
            const int nb = std::min(chunk, B - b0);
            const float* d_preds = preds + (size_t)b0 * PN;
            if (!device) {
                HIPCHK(h, hipMemcpyAsync(h->d_bme_preds, d_preds, (size_t)nb * PN * sizeof(float), hipMemcpyHostToDevice, h->stream));
                d_preds = h->d_bme_preds;
            }
            if ((rc = bme_chunk(h, spr, d_preds, io.start + (size_t)b0 * T, nb, N, io.slots + (size_t)b0 * T, io.lengths + (size_t)b0 * T,
                                io.steps + b0, io.tree_length + b0, io.status + b0)))
                return rc;
        }
        if (device) {
            if ((rc = list_copy(h, list, false, hipMemcpyHostToDevice))) return rc;
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
    } catch (const std::bad_alloc&) { return fail(h, PF_ENOMEM, "out of host memory for the tables of N=%d sequences", N); }
    return PF_OK;
}

// ---- split supports of join tables (pf_join_supports, pf_join_supports_device; pf_support.hip.h) ----

static_assert(pfbme::MAX_N <= 64 * pfsup::MAX_W, "k_sup_match keeps TILE splits of MAX_W words in LDS");
// (state_bytes: the least a call needs - a source's reference table and one replicate table; the plan below sizes chunks)
const TreeSearch SUP_SEARCH{"split supports", pfbme::MAX_N, pfsup::min_state_bytes, pfsup::SUP_MAX_Y,
                            "the bitset tables of the reference and of one replicate"};
// pf_join_transfers: one more int32 per (replicate, split), the key beside the delta
const TreeSearch TRANSFER_SEARCH{"transfer counts", pfbme::MAX_N, pfsup::min_transfer_state_bytes, pfsup::SUP_MAX_Y,
                                 "the bitset tables of the reference and of one replicate, its deltas and keys"};

// The chunks of a call: `nb` whole sources side by side where a source's R + 1 tables and its delta fit the workspace
// limit, otherwise one source at a time in runs of `rc` replicates.  Refused only where the reference and one replicate
// do not fit (check_tree_shape names the bytes).
int plan_supports(pf_handle* h, int B, int R, int N, int* nb, int* rc, bool arg = false) {
    int chunk = 0;
    const int rc0 = check_tree_shape(h, arg ? TRANSFER_SEARCH : SUP_SEARCH, B, N, &chunk);
    if (rc0) return rc0;
    if (N < 4) return fail(h, PF_EINVAL, "split supports need N >= 4 sequences (got %d): a tree of 3 has no split", N);
    if (R < 1) return fail(h, PF_EINVAL, "split supports need R >= 1 replicates (got %d)", R);
    size_t n = 0;
    if (!mul_size((size_t)B, (size_t)R, (size_t)pfnj::table_len(N) * sizeof(int32_t), &n))
        return fail(h, PF_EINVAL, "B=%d sources of R=%d replicate tables overflow the address space", B, R);
    // (a launch's workgroups times their 256 threads stay below 2^32)
    const int64_t tiles = ((int64_t)N - 3 + pfsup::TILE - 1) / pfsup::TILE, max_trees = std::max<int64_t>(2, ((int64_t)1 << 23) / tiles);
    const size_t limit = (size_t)h->ws_limit_bytes, per = arg ? pfsup::transfer_state_bytes(N, R) : pfsup::state_bytes(N, R);
    if (per <= limit && (int64_t)R + 1 <= max_trees && R <= pfsup::SUP_MAX_Y) {
        *rc = R;
        *nb = (int)std::min<int64_t>(std::min<int64_t>(B, pfsup::SUP_MAX_Y), std::min<int64_t>((int64_t)(limit / per), max_trees / ((int64_t)R + 1)));
        return PF_OK;
    }
    const size_t tree = pfsup::tree_bytes(N), each = tree + (arg ? 2 : 1) * pfsup::sizes_bytes(N);      // (limit >= state_bytes(N, 1): checked)
    *nb = 1;
    *rc = (int)std::min<int64_t>(std::min<int64_t>(R, pfsup::SUP_MAX_Y), std::min<int64_t>((int64_t)((limit - tree - pfsup::sizes_bytes(N)) / each), max_trees - 1));
    return PF_OK;
}

// all chunks of a call on device arrays `d`, enqueued on h->stream; `transfers`: pf_join_transfers' results too
int supports_launch(pf_handle* h, const pfsup::Tables& d, int B, int R, int N, int nb, int rc, bool transfers, int cutoff) {
    int rc2 = h->d_sup.reserve(h, (size_t)nb * (transfers ? pfsup::transfer_state_bytes(N, rc) : pfsup::state_bytes(N, rc)));
    if (rc2) return rc2;
    if ((rc2 = h->d_sup_bad.reserve(h, (size_t)B * ((size_t)R + 1)))) return rc2;
    h->cur = h->stream;
    HIPCHK(h, hipMemsetAsync(h->d_sup_bad, 0, (size_t)B * ((size_t)R + 1), h->stream));
    pfsup::Args a{};
    a.ref_slots = d.ref; a.rep_slots = d.rep; a.rep_flag = d.flag; a.bad = h->d_sup_bad;
    a.count = d.count; a.transfer = d.transfer; a.depth = d.depth; a.status = d.status;
    a.N = N; a.R = R;
    pfsup::Transfers x{nullptr, d.moves, d.used, d.capped, d.branch, cutoff};
    pfsup::Transfers* const more = transfers ? &x : nullptr;
    // (chunks follow each other on the stream, so the next one may reuse the state)
    for (int b0 = 0; b0 < B; b0 += nb)
        for (int r0 = 0; r0 < R; r0 += rc) {
            a.b0 = b0; a.nb = std::min(nb, B - b0); a.r0 = r0; a.rc = std::min(rc, R - r0);
            pfsup::carve(a, h->d_sup, more);
            const hipError_t e = pfsup::launch_chunk(h->stream, a, r0 == 0, more);
            if (e != hipSuccess) return fail(h, PF_EHIP, "k_sup_* launch failed: %s", hipGetErrorString(e));
        }
    return PF_OK;
}

// The tables of a host call, validated as a start table is (a replicate passed with its flag is never read: its table
// may be anything); ref: pf_join_supports' and pf_join_transfers' reference tables, null for pf_join_consensus
int check_join_tables(pf_handle* h, const int32_t* ref, const int32_t* rep, const uint8_t* flag, int B, int R, int N) {
    const size_t T = (size_t)pfnj::table_len(N), b = (size_t)B, r = (size_t)R;
    try {
        const int rc = ref ? check_bme_starts(h, ref, B, N) : PF_OK;
        if (rc) return rc;
        std::vector<int32_t> parent((size_t)pfbme::nodes_of(N)), children((size_t)pfbme::nodes_of(N) * 3);
        for (size_t i = 0; i < b * r; ++i)
            if (!(flag && flag[i]) && !pfbme::tree_of_joins(rep + i * T, N, parent.data(), children.data()))
                return fail(h, PF_EINVAL, "source %zu: replicate %zu is not a join table of N=%d sequences", i / r, i % r, N);
    } catch (const std::bad_alloc&) { return fail(h, PF_ENOMEM, "out of host memory for the tables of N=%d sequences", N); }
    return PF_OK;
}

// pf_join_transfers' own refusal, before the shared ones
int check_cutoff(pf_handle* h, int cutoff) {
    if (cutoff < 0 || cutoff > 100) return fail(h, PF_EINVAL, "the transfer cutoff is a percent from 0 to 100 (got %d)", cutoff);
    return PF_OK;
}

// pf_join_supports or, `transfers`, pf_join_transfers (the same call with its Transfers part);
// the caller's arrays on the device (asynchronous) or on the host
int supports_impl(pf_handle* h, bool transfers, bool device, const pfsup::Tables& user, int B, int R, int N, int cutoff) {
    pfsup::Tables io{};
    auto list = [&](auto& v) { pfsup::staging_arrays(v, io, user, (size_t)B, (size_t)R, N, transfers, user.branch != nullptr); };
    if (pfspan::missing(list)) return fail(h, PF_EINVAL, "null buffer");
    int nb = 0, rc = 0;
    int rc2 = transfers ? check_cutoff(h, cutoff) : PF_OK;
    if (rc2 || (rc2 = plan_supports(h, B, R, N, &nb, &rc, transfers))) return rc2;
    if (!device) {
        size_t n = 0;
        if (user.branch && !mul_size((size_t)B * ((size_t)N - 3), (size_t)N, sizeof(int32_t), &n))
            return fail(h, PF_EINVAL, "B=%d tables of branch moves of N=%d sequences overflow the address space", B, N);
        if ((rc2 = check_join_tables(h, user.ref, user.rep, user.flag, B, R, N))) return rc2;
    }
    HIPCHK(h, hipSetDevice(h->device));
    ++(transfers ? h->transfer_calls : h->sup_calls);
    if (device) return supports_launch(h, user, B, R, N, nb, rc, transfers, cutoff);
    return staged_call(h, h->d_sup_io, list, [&] { return supports_launch(h, io, B, R, N, nb, rc, transfers, cutoff); });
}

// ---- majority-rule consensus of replicate join tables (pf_join_consensus, pf_join_consensus_device; pf_consensus.hip.h,
// DESIGN.md section 25) ----

static_assert(pfbme::MAX_N <= 64 * pfcon::MAX_W, "k_con_nest keeps TILE splits of MAX_W words in LDS");
// (state_bytes: the least a call needs - a source of one replicate; the plan below sizes a source of R)
const TreeSearch CON_SEARCH{"majority-rule consensus", pfbme::MAX_N, pfcon::min_state_bytes, pfcon::CON_MAX_Y,
                            "the bitset table of one replicate and its hash table"};

// The chunks of a call: `nb` whole sources side by side.  A source always runs whole - the owners' bitsets must outlive
// the counting -, so one whose R tables, hash table and [M][R] lengths exceed the workspace limit is refused.
int plan_consensus(pf_handle* h, int B, int R, int N, int percent, int* nb) {
    int chunk = 0;
    const int rc0 = check_tree_shape(h, CON_SEARCH, B, N, &chunk);
    if (rc0) return rc0;
    if (N < 4) return fail(h, PF_EINVAL, "a consensus needs N >= 4 sequences (got %d): a tree of 3 has no split", N);
    if (R < 1) return fail(h, PF_EINVAL, "a consensus needs R >= 1 replicates (got %d)", R);
    if (percent < 50 || percent > 99) return fail(h, PF_EINVAL, "the consensus threshold is a percent from 50 to 99 (got %d)", percent);
    size_t n = 0;
    if (!mul_size((size_t)B, (size_t)R, (size_t)pfnj::table_len(N) * sizeof(double), &n))
        return fail(h, PF_EINVAL, "B=%d sources of R=%d replicate tables overflow the address space", B, R);
    if ((int64_t)R * ((int64_t)N - 3) > pfcon::MAX_ENTRIES || R > pfcon::CON_MAX_Y)
        return fail(h, PF_EINVAL, "R=%d replicates of N=%d sequences are more than %d trees or %lld splits of one source", R, N,
                    pfcon::CON_MAX_Y, (long long)pfcon::MAX_ENTRIES);
    const size_t per = pfcon::state_bytes(N, R);
    if ((int64_t)per > h->ws_limit_bytes)
        return fail(h, PF_EINVAL, "majority-rule consensus of R=%d replicates of N=%d sequences needs %zu bytes of state per source (its "
                                  "R bitset tables, hash table and [M][R] lengths; a source runs whole), above the workspace limit of "
                                  "%lld bytes (option ws_limit_mb)", R, N, per, (long long)h->ws_limit_bytes);
    *nb = (int)std::min<size_t>((size_t)std::min(B, pfcon::CON_MAX_Y), (size_t)h->ws_limit_bytes / per);
    return PF_OK;
}

// all chunks of a call on device arrays `d`, enqueued on h->stream
int consensus_launch(pf_handle* h, const pfcon::Tables& d, int B, int R, int N, int percent, int nb) {
    const int rc2 = h->d_con.reserve(h, (size_t)nb * pfcon::state_bytes(N, R));
    if (rc2) return rc2;
    h->cur = h->stream;
    const size_t S = (size_t)N - 3, b = (size_t)B;
    // (the first M entries are written; beyond them, and for a source with a status, the results are zeros)
    HIPCHK(h, hipMemsetAsync(d.n_splits, 0, b * sizeof(int32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(d.count, 0, b * S * sizeof(int32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(d.size, 0, b * S * sizeof(int32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(d.parent, 0, b * S * sizeof(int32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(d.leaf_parent, 0, b * (size_t)N * sizeof(int32_t), h->stream));
    if (d.lengths) {
        HIPCHK(h, hipMemsetAsync(d.split_length, 0, b * S * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(d.leaf_length, 0, b * (size_t)N * sizeof(double), h->stream));
    }
    pfcon::Args a{};
    a.rep_slots = d.rep; a.rep_lengths = d.lengths; a.rep_flag = d.flag;
    a.n_splits = d.n_splits; a.count = d.count; a.size = d.size; a.parent = d.parent; a.leaf_parent = d.leaf_parent;
    a.split_length = d.split_length; a.leaf_length = d.leaf_length; a.status = d.status;
    a.N = N; a.R = R; a.percent = percent;
    a.cap = pfcon::capacity_of((int64_t)R * ((int64_t)N - 3));
    // (chunks follow each other on the stream, so the next one may reuse the state)
    for (int b0 = 0; b0 < B; b0 += nb) {
        a.b0 = b0; a.nb = std::min(nb, B - b0);
        const pfcon::Fill f = pfcon::carve(a, h->d_con);
        const hipError_t e = pfcon::launch_chunk(h->stream, a, f);
        if (e != hipSuccess) return fail(h, PF_EHIP, "k_con_* launch failed: %s", hipGetErrorString(e));
    }
    return PF_OK;
}

// the caller's arrays on the device (asynchronous) or on the host
int consensus_impl(pf_handle* h, bool device, const pfcon::Tables& user, int B, int R, int N, int percent) {
    pfcon::Tables io{};
    auto list = [&](auto& v) { pfcon::staging_arrays(v, io, user, (size_t)B, (size_t)R, N); };
    if (pfspan::missing(list)) return fail(h, PF_EINVAL, "null buffer");
    int nb = 0;
    int rc2 = plan_consensus(h, B, R, N, percent, &nb);
    if (rc2 || (!device && (rc2 = check_join_tables(h, nullptr, user.rep, user.flag, B, R, N)))) return rc2;
    HIPCHK(h, hipSetDevice(h->device));
    ++h->con_calls;
    if (device) return consensus_launch(h, user, B, R, N, percent, nb);
    return staged_call(h, h->d_con_io, list, [&] { return consensus_launch(h, io, B, R, N, percent, nb); });
}

// ---- distances between the join tables of a source (pf_join_distances, pf_join_distances_device; pf_treedist.hip.h,
// DESIGN.md section 35) ----

static_assert(pftd::MAX_N == pfbme::MAX_N, "a table that pf_bme_nni takes is one pf_join_distances takes");
// (state_bytes: the least a call needs - a source of one tree; the plan below sizes a source of K)
const TreeSearch TD_SEARCH{"tree distances", pftd::MAX_N, pftd::min_state_bytes, pftd::TD_MAX_Y,
                           "the bitset table of one tree and its hash table"};

// The chunks of a call: `nb` whole sources side by side.  A source always runs whole - every pair needs both trees'
// indices into one hash table -, so one whose K tables and hash table exceed the workspace limit is refused.
int plan_distances(pf_handle* h, int B, int K, int N, int* nb) {
    if (N < 4) return fail(h, PF_EINVAL, "tree distances need N >= 4 sequences (got %d): a tree of 3 has no split", N);
    int chunk = 0;
    const int rc0 = check_tree_shape(h, TD_SEARCH, B, N, &chunk);
    if (rc0) return rc0;
    if (K < 1) return fail(h, PF_EINVAL, "tree distances need K >= 1 trees (got %d)", K);
    if (K > pftd::MAX_K) return fail(h, PF_EINVAL, "tree distances take at most %d trees of one source (got K=%d)", pftd::MAX_K, K);
    size_t n = 0;
    if (!mul_size((size_t)B, (size_t)K, (size_t)pfnj::table_len(N) * sizeof(double), &n) ||
        !mul_size((size_t)B, (size_t)K * (size_t)K, sizeof(double), &n))
        return fail(h, PF_EINVAL, "B=%d sources of K=%d trees overflow the address space", B, K);
    const size_t per = pftd::state_bytes(N, K);
    if ((int64_t)per > h->ws_limit_bytes)
        return fail(h, PF_EINVAL, "tree distances of K=%d trees of N=%d sequences need %zu bytes of state per source (its K bitset "
                                  "tables, their indices and the hash table; a source runs whole), above the workspace limit of "
                                  "%lld bytes (option ws_limit_mb)", K, N, per, (long long)h->ws_limit_bytes);
    *nb = (int)std::min<size_t>((size_t)std::min(B, pftd::TD_MAX_Y), (size_t)h->ws_limit_bytes / per);
    return PF_OK;
}

// all chunks of a call on device arrays `d`, enqueued on h->stream
int distances_launch(pf_handle* h, const pftd::Tables& d, int B, int K, int N, int nb) {
    const int rc2 = h->d_td.reserve(h, (size_t)nb * pftd::state_bytes(N, K));
    if (rc2) return rc2;
    h->cur = h->stream;
    const size_t cells = (size_t)B * (size_t)K * (size_t)K;
    // (a source with a status keeps these zeros)
    HIPCHK(h, hipMemsetAsync(d.shared, 0, cells * sizeof(int32_t), h->stream));
    if (d.lengths) {
        HIPCHK(h, hipMemsetAsync(d.kf, 0, cells * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(d.wrf, 0, cells * sizeof(double), h->stream));
    }
    pftd::Args a{};
    a.c.rep_slots = d.slots; a.c.rep_lengths = d.lengths; a.c.rep_flag = d.flag; a.c.status = d.status;
    a.c.N = N; a.c.R = K;
    a.c.cap = pfcon::capacity_of((int64_t)K * ((int64_t)N - 3));
    a.shared = d.shared; a.kf = d.kf; a.wrf = d.wrf;
    // (chunks follow each other on the stream, so the next one may reuse the state)
    for (int b0 = 0; b0 < B; b0 += nb) {
        a.c.b0 = b0; a.c.nb = std::min(nb, B - b0);
        const pfcon::Fill f = pftd::carve(a, h->d_td);
        const hipError_t e = pftd::launch_chunk(h->stream, a, f);
        if (e != hipSuccess) return fail(h, PF_EHIP, "k_td_* launch failed: %s", hipGetErrorString(e));
    }
    return PF_OK;
}

// the caller's arrays on the device (asynchronous) or on the host
int distances_impl(pf_handle* h, bool device, const pftd::Tables& user, int B, int K, int N) {
    pftd::Tables io{};
    auto list = [&](auto& v) { pftd::staging_arrays(v, io, user, (size_t)B, (size_t)K, N); };
    if (pfspan::missing(list)) return fail(h, PF_EINVAL, "null buffer");
    int nb = 0;
    int rc2 = plan_distances(h, B, K, N, &nb);
    if (rc2 || (!device && (rc2 = check_join_tables(h, nullptr, user.slots, user.flag, B, K, N)))) return rc2;
    HIPCHK(h, hipSetDevice(h->device));
    ++h->td_calls;
    if (device) return distances_launch(h, user, B, K, N, nb);
    return staged_call(h, h->d_td_io, list, [&] { return distances_launch(h, io, B, K, N, nb); });
}

}  // namespace

extern "C" {

int pf_abi_version(void) { return PF_ABI_VERSION; }

uint64_t pf_blob_len(int32_t n_blocks, int32_t n_heads, int32_t embed_dim) {
    return read_blob(nullptr, n_blocks, embed_dim, n_heads).len;
}

// device + stream, no weights yet
static int open_device(int device, pf_handle** out) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(nullptr, PF_EHIP, "no HIP device available (%s); there is no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (device < 0 || device >= ndev) return fail(nullptr, PF_EINVAL, "device %d out of range (have %d)", device, ndev);
    pf_handle* h = new pf_handle();
    if (const char* e = getenv("PF_TWO_STREAMS")) h->two_streams = atoi(e) != 0;   // A/B runs of whole programs
    if (getenv("PF_ROW_TILES")) h->tile_force = 0;          // read once: the tiling (and with it the layout of
    if (getenv("PF_FLAT_TILES")) h->tile_force = 1;
    if (const char* v = getenv("PF_COLSTATS_RING")) h->colstats_ring = atoi(v) != 0;   // A/B and counter runs (tools/pmc_colstats.sh)         // spart / outpart) cannot change between two calls
    h->device = device;
    int rc = PF_OK;
    do {
        if ((e = hipSetDevice(device)) != hipSuccess) { rc = fail(nullptr, PF_EHIP, "hipSetDevice: %s", hipGetErrorString(e)); break; }
        if ((e = hipGetDeviceProperties(&h->prop, device)) != hipSuccess) { rc = fail(nullptr, PF_EHIP, "hipGetDeviceProperties: %s", hipGetErrorString(e)); break; }
        if (std::string(h->prop.gcnArchName).rfind("gfx950", 0) != 0) {
            rc = fail(nullptr, PF_EHIP, "device %d is %s; this library is built for gfx950 only", device, h->prop.gcnArchName);
            break;
        }
        if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) { rc = fail(nullptr, PF_EHIP, "hipStreamCreate: %s", hipGetErrorString(e)); break; }
        h->cur = h->stream;
        if ((e = hipHostMalloc((void**)&h->bad_idx_host, 3 * sizeof(unsigned), hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess ||
            (e = hipHostGetDevicePointer((void**)&h->bad_idx_dev, h->bad_idx_host, 0)) != hipSuccess) {
            rc = fail(nullptr, PF_EHIP, "hipHostMalloc (residue flag): %s", hipGetErrorString(e));
            break;
        }
        h->bad_idx_host[0] = h->bad_idx_host[1] = h->bad_idx_host[2] = 0u;
        // Kernels that need more than the default 64 KB of dynamic LDS: the attribute is set here, once per
        // handle and before any launch, so that no launch path carries mutable state shared between handles
        // (the CLI drives two engines per GPU from two host threads).
        auto big_lds = [&](const void* fn, int bytes) {
            if (!rc && (e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes)) != hipSuccess)
                rc = fail(nullptr, PF_EHIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
        };
        for (const MainRow& r : main_kernels())       // (k_main over every alignment; the routed launches run without it)
            if (r.kind.route == ROUTE_ALL) big_lds(reinterpret_cast<const void*>(r.fn), MAIN_LDS_BYTES);
        big_lds(reinterpret_cast<const void*>(&k_row_stats), ROW_STATS_LDS_BYTES);
        big_lds(reinterpret_cast<const void*>(&k_embed<false>), EMBED_LDS_BYTES);
        big_lds(reinterpret_cast<const void*>(&k_embed<true>), EMBED_LDS_BYTES);
        big_lds(reinterpret_cast<const void*>(&pffit::k_fit_setup), pffit::SETUP_LDS_MAX);
        big_lds(reinterpret_cast<const void*>(&pffit::k_fit_pairs<true>), pffit::LDS_MAX_BYTES);
        big_lds(reinterpret_cast<const void*>(&pfols::k_ols_setup), pfols::SETUP_LDS_MAX);
        if (rc) break;
    } while (0);
    if (rc) { pf_destroy(h); return rc; }
    *out = h;
    return PF_OK;
}

int pf_create_bare(int device, pf_handle_t** out) {
    if (!out) return fail(nullptr, PF_EINVAL, "null argument");
    *out = nullptr;
    return open_device(device, out);
}

int pf_create(const pf_weights_t* w, int device, pf_handle_t** out) {
    if (!w || !out || !w->blob) return fail(nullptr, PF_EINVAL, "null argument");
    *out = nullptr;
    // (refused before any device access: the rule holds on a machine without a GPU too)
    if (!generic_arch_ok(w))
        return fail(nullptr, PF_EINVAL,
                    "unsupported architecture: n_blocks=%d n_heads=%d embed_dim=%d n_alphabet=%d "
                    "(n_alphabet must be 22, n_blocks 1..64, embed_dim must be 1..256 and divisible by n_heads)",
                    w->n_blocks, w->n_heads, w->embed_dim, w->n_alphabet);
    if (w->blob_len != pf_blob_len(w->n_blocks, w->n_heads, w->embed_dim))
        return fail(nullptr, PF_EINVAL, "weight blob has %llu floats, expected %llu",
                    (unsigned long long)w->blob_len,
                    (unsigned long long)pf_blob_len(w->n_blocks, w->n_heads, w->embed_dim));
    pf_handle* h = nullptr;
    int rc = open_device(device, &h);
    if (rc) return rc;
    h->n_blocks = w->n_blocks;
    h->garch = pfg::make_arch(w->embed_dim, w->n_heads);
    const BlobView bv = read_blob(w->blob, w->n_blocks, w->embed_dim, w->n_heads);
    if (w->embed_dim == E && w->n_heads == NH) {
        // the default and precise kernels; the generic image waits for the first forward with option "generic" = 1
        rc = prepare_weights(h, bv, w->blob_len);
        if (!rc) rc = prepare_precise_weights(h, bv, &h->pw);
        if (!rc) {
            try { h->blob_copy.assign(w->blob, w->blob + w->blob_len); }
            catch (const std::bad_alloc&) { rc = fail(h, PF_ENOMEM, "out of host memory copying the weights"); }
        }
    } else {
        h->arch_generic = true;          // the kernels of the other two paths are specialised for (64, 4)
        rc = prepare_generic_weights(h, bv);
    }
    if (rc) g_create_error = h->err;
    if (rc) { pf_destroy(h); return rc; }
    *out = h;
    return PF_OK;
}

int pf_destroy(pf_handle_t* h) {
    if (!h) return PF_OK;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->stream2) hipStreamSynchronize(h->stream2);
    for (void*& c : h->comm) if (c && g_rccl.CommDestroy) { g_rccl.CommDestroy(c); c = nullptr; }
    for (auto& s : h->pending) { hipEventDestroy(s.a); hipEventDestroy(s.b); }
    for (auto e : h->free_events) hipEventDestroy(e);
    for (void* p : h->owned) hipFree(p);
    for (DeviceBuffer* b : h->buffers) b->release();
    if (h->stream2) hipStreamDestroy(h->stream2);
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    if (h->ev_join) hipEventDestroy(h->ev_join);
    if (h->stream) hipStreamDestroy(h->stream);
    if (h->bad_idx_host) hipHostFree(h->bad_idx_host);
    delete h;
    return PF_OK;
}

const char* pf_last_error(const pf_handle_t* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int pf_set_option(pf_handle_t* h, const char* key, int64_t value) {
    if (!h || !key) return PF_EINVAL;
    const std::string k(key);
    if (k == "max_seqs") h->max_seqs = value;
    else if (k == "profile") { drain_profile(h); h->profile = value != 0; h->profile_main_only = value == 2; }
    else if (k == "debug_keep") h->debug_keep = value != 0;
    else if (k == "embed_mfma") h->embed_mfma = value != 0;
    else if (k == "colstats_fine") h->colstats_fine = value < 0 ? -1 : (value != 0);
    else if (k == "materialize_x0") h->materialize_x0 = value != 0;
    else if (k == "overlap") h->overlap = value != 0;
    else if (k == "two_streams") h->two_streams = value != 0;
    else if (k == "reserve_cus") h->reserve_cus = (int)std::max<int64_t>(0, std::min<int64_t>(value, 128));
    else if (k == "ablate") h->ablate = (int)value;
    else if (k == "head_fold") h->head_fold = value != 0;
    else if (k == "force_rccl") h->force_rccl = value != 0;
    else if (k == "colstats_ring") h->colstats_ring = value != 0;
    else if (k == "site_dedup") h->site_dedup = value != 0;
    else if (k == "main_dedup") h->main_dedup = value <= 0 ? 0 : (value >= 2 ? 2 : 1);
    else if (k == "stats_dedup") h->stats_dedup = value != 0;
    else if (k == "precise") h->precise = value < 0 ? -1 : (value != 0);
    else if (k == "recheck_above") h->recheck_above = value > 0 ? (double)value : 0.0;
    else if (k == "precise_ffn_valu") h->precise_ffn_valu = value != 0;
    else if (k == "generic") {
        if (h->arch_generic && !value)
            return fail(h, PF_EINVAL, "embed_dim %d / n_heads %d runs on the generic kernels only (option generic cannot be 0)",
                        h->garch.E, h->garch.NH);
        h->generic = value != 0;
    }
    else if (k == "phase_prof") {
        if (value && !h->phase_prof) { HIPCHK(h, hipMalloc((void**)&h->phase_prof, 64)); h->owned.push_back(h->phase_prof); }
        if (h->phase_prof) HIPCHK(h, hipMemset(h->phase_prof, 0, 64));
        if (!value) h->phase_prof = nullptr;
        h->phase_prof_last = value == 2;
    }
    else if (k == "ws_limit_mb") h->ws_limit_bytes = value << 20;
    else if (k == "spr_pairs_simple") h->spr_pairs_simple = value != 0;
    else if (k == "delta_atomic") h->delta_atomic = value != 0;
    else if (k == "fit_lds_bytes") h->fit_lds_bytes = value > 0 ? std::min<int64_t>(value, pffit::LDS_MAX_BYTES) : pffit::LDS_MAX_BYTES;
    else if (k == "spr_step_cap") h->spr_step_cap = value > 0 ? value : 0;
    else if (k == "sub_floats") h->sub_floats = value > 0 ? value : SUB_FLOATS_DEFAULT;
    else return fail(h, PF_EINVAL, "unknown option '%s'", key);
    return PF_OK;
}

int pf_forward(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, float* out) {
    if (!h) return PF_EINVAL;
    return forward_host_impl(h, idx, B, N, 0, L, L, out);
}

int pf_resample_sites_device(pf_handle_t* h, const uint8_t* d_src, int32_t B, int32_t N, int32_t L, int32_t r_begin, int32_t R,
                             uint64_t seed, uint8_t* d_dst) {
    if (!h) return PF_EINVAL;
    if (!d_src || !d_dst) return fail(h, PF_EINVAL, "null buffer");
    if (B < 1 || N < 1 || L < 1 || R < 1 || r_begin < 0)
        return fail(h, PF_EINVAL, "bad dimensions B=%d N=%d L=%d r_begin=%d R=%d", B, N, L, r_begin, R);
    size_t n = 0;
    if (!mul_size((size_t)B, (size_t)R, (size_t)N * L, &n))
        return fail(h, PF_EINVAL, "B=%d x R=%d replicates of %d x %d overflow the address space", B, R, N, L);
    HIPCHK(h, hipSetDevice(h->device));
    return launch_resample(h, d_src, B, N, L, r_begin, R, seed, d_dst);
}

int pf_bootstrap(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, int32_t R, uint64_t seed, float* out) {
    if (!h) return PF_EINVAL;
    return bootstrap_impl(h, idx, B, N, L, R, seed, out);
}

int pf_window_count(int32_t L, int32_t W, int32_t step) {
    const int n = pfsites::window_count(L, W, step);
    return n < 0 ? PF_EINVAL : n;
}

int pf_window_start(int32_t L, int32_t W, int32_t step, int32_t s) {
    const int st = pfsites::window_start(L, W, step, s);
    return st < 0 ? PF_EINVAL : st;
}

int pf_gather_sites_device(pf_handle_t* h, const uint8_t* d_src, int32_t B, int32_t N, int32_t L, const int32_t* d_sites,
                           const int32_t* d_start, int32_t S, int32_t K, uint8_t* d_dst) {
    if (!h) return PF_EINVAL;
    if (!d_src || !d_dst) return fail(h, PF_EINVAL, "null buffer");
    if (!d_sites == !d_start) return fail(h, PF_EINVAL, "exactly one of d_sites (table) and d_start (affine) must be given");
    if (B < 1 || N < 1 || L < 1 || S < 1 || K < 1 || K > L)
        return fail(h, PF_EINVAL, "bad dimensions B=%d N=%d L=%d S=%d K=%d (1 <= K <= L)", B, N, L, S, K);
    size_t n = 0;
    if (!mul_size((size_t)B, (size_t)S, (size_t)N * K, &n) || !mul_size((size_t)S, (size_t)K, sizeof(int32_t), &n))
        return fail(h, PF_EINVAL, "B=%d x S=%d site sets of %d x %d overflow the address space", B, S, N, K);
    HIPCHK(h, hipSetDevice(h->device));
    return launch_gather(h, d_src, B, N, L, d_sites, d_start, 0, S, K, d_dst);
}

int pf_forward_sites(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, const int32_t* sites, int32_t S,
                     int32_t K, float* out) {
    if (!h) return PF_EINVAL;
    if (!sites) return fail(h, PF_EINVAL, "null buffer");
    return sites_impl(h, idx, B, N, L, sites, 0, S, K, out);
}

int pf_forward_windows(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, int32_t W, int32_t step, float* out,
                       int32_t S_cap) {
    if (!h) return PF_EINVAL;
    if (step < 1) return fail(h, PF_EINVAL, "windows need step >= 1 (got %d)", step);
    int rc = check_dims(h, B, N, L, L);
    if (rc) return rc;
    if (W < 1 || W > L) return fail(h, PF_EINVAL, "a site set needs 1 <= K <= L sites (got K=%d, L=%d)", W, L);
    const int S = pfsites::window_count(L, W, step);
    if (S < 0) return fail(h, PF_EINVAL, "bad window rule L=%d W=%d step=%d", L, W, step);
    if (S_cap < S) return fail(h, PF_EINVAL, "out holds %d windows, L=%d W=%d step=%d gives %d", S_cap, L, W, step, S);
    return sites_impl(h, idx, B, N, L, nullptr, step, S, W, out);
}

int pf_gather_taxa_device(pf_handle_t* h, const uint8_t* d_src, int32_t B, int32_t N, int32_t L, const int32_t* d_taxa, int32_t S,
                          int32_t M, uint8_t* d_dst) {
    if (!h) return PF_EINVAL;
    if (!d_src || !d_dst || !d_taxa) return fail(h, PF_EINVAL, "null buffer");
    if (B < 1 || N < 1 || L < 1 || S < 1 || M < 1) return fail(h, PF_EINVAL, "bad dimensions B=%d N=%d L=%d S=%d M=%d", B, N, L, S, M);
    size_t n = 0;
    if (!mul_size((size_t)B, (size_t)S, (size_t)M * L, &n) || !mul_size((size_t)S, (size_t)M, sizeof(int32_t), &n) ||
        !mul_size((size_t)B, (size_t)N, (size_t)L, &n))
        return fail(h, PF_EINVAL, "B=%d x S=%d taxon sets of %d x %d overflow the address space", B, S, M, L);
    HIPCHK(h, hipSetDevice(h->device));
    return launch_gather_taxa(h, d_src, B, N, L, d_taxa, 0, S, M, d_dst);
}

int pf_forward_taxa(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, const int32_t* taxa, int32_t S, int32_t M,
                    float* out) {
    if (!h) return PF_EINVAL;
    return taxa_impl(h, idx, B, N, L, taxa, S, M, out);
}

int pf_forward_leave_one_out(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, float* out, float* loo,
                             float* influence, float* shift, float* context) {
    if (!h) return PF_EINVAL;
    return loo_impl(h, idx, B, N, L, out, loo, influence, shift, context);
}

int pf_loo_stats_device(pf_handle_t* h, const float* d_full, const float* d_loo, int32_t B, int32_t N, float* d_influence,
                        float* d_shift, float* d_context) {
    if (!h) return PF_EINVAL;
    if (!d_full || !d_loo || !d_influence || !d_shift || !d_context) return fail(h, PF_EINVAL, "null buffer");
    if (B < 1 || N < 3 || N > 32767) return fail(h, PF_EINVAL, "bad dimensions B=%d N=%d (leave-one-out needs 3 <= N <= 32767)", B, N);
    size_t n = 0;
    if (!mul_size((size_t)B, (size_t)N, (size_t)(N - 1) * (N - 2) / 2 * sizeof(float), &n))
        return fail(h, PF_EINVAL, "B=%d x %d leave-one-out sets of %d sequences overflow the address space", B, N, N - 1);
    HIPCHK(h, hipSetDevice(h->device));
    return launch_loo_stats(h, d_full, d_loo, B, N, d_influence, d_shift, d_context);
}

int pf_forward_place(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t M, int32_t L, int32_t Q, float* out, float* base,
                     float* sets, float* place, float* disturb, float* shift, float* joint) {
    if (!h) return PF_EINVAL;
    return place_impl(h, idx, B, M, L, Q, out, base, sets, place, disturb, shift, joint);
}

int pf_place_stats_device(pf_handle_t* h, const float* d_whole, const float* d_base, const float* d_sets, int32_t B, int32_t N,
                          int32_t Q, float* d_place, float* d_disturb, float* d_shift, float* d_joint) {
    if (!h) return PF_EINVAL;
    if (!d_whole || !d_base || !d_sets || !d_place || !d_disturb || !d_shift || !d_joint) return fail(h, PF_EINVAL, "null buffer");
    if (B < 1 || N < 2 || Q < 1 || (int64_t)N + Q > 32767)
        return fail(h, PF_EINVAL, "bad dimensions B=%d N=%d Q=%d (placement needs N >= 2, Q >= 1, N + Q <= 32767)", B, N, Q);
    size_t n = 0;
    if (!mul_size((size_t)B, (size_t)Q, (size_t)(N + 1) * N / 2 * sizeof(float), &n) ||
        !mul_size((size_t)B, (size_t)(N + Q) * (N + Q - 1) / 2, sizeof(float), &n))
        return fail(h, PF_EINVAL, "B=%d x %d query sets of %d sequences overflow the address space", B, Q, N + 1);
    HIPCHK(h, hipSetDevice(h->device));
    return launch_place_stats(h, d_whole, d_base, d_sets, B, N, Q, d_place, d_disturb, d_shift, d_joint);
}

int pf_tile_groups(int32_t N, int32_t M) {
    const int64_t g = pftile::groups(N, M);
    return g < 0 ? PF_EINVAL : (int)g;
}

int pf_tile_bound(int32_t N, int32_t M, int32_t g) {
    const int64_t G = pftile::groups(N, M);
    if (G < 0 || g < 0 || g > G) return PF_EINVAL;
    return (int)pftile::bound(N, G, g);
}

int pf_forward_tiled(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, int32_t M, float* out, float* spread) {
    if (!h) return PF_EINVAL;
    return tiled_impl(h, idx, B, N, L, M, out, spread);
}

int pf_tile_combine_device(pf_handle_t* h, const float* d_sets, int32_t B, int32_t N, int32_t M, float* d_out, float* d_spread) {
    if (!h) return PF_EINVAL;
    if (!d_sets || !d_out || !d_spread) return fail(h, PF_EINVAL, "null buffer");
    int rc = check_tiled_shape(h, B, N, M);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = ensure_tiled_plan(h, N, M))) return rc;
    size_t n = 0;
    if (!mul_size((size_t)B, (size_t)h->tiled_plan.T, sizeof(float), &n))
        return fail(h, PF_EINVAL, "B=%d x %lld set distances overflow the address space", B, (long long)h->tiled_plan.T);
    return launch_tile_combine(h, d_sets, B, d_out, d_spread);
}

int pf_nj_joins(pf_handle_t* h, const float* preds, int32_t B, int32_t N, int32_t* slots, double* lengths, uint8_t* nonfinite) {
    if (!h) return PF_EINVAL;
    return nj_impl(h, false, false, {preds, slots, lengths, nonfinite}, B, N);
}

int pf_nj_joins_device(pf_handle_t* h, const float* d_preds, int32_t B, int32_t N, int32_t* d_slots, double* d_lengths,
                       uint8_t* d_nonfinite) {
    if (!h) return PF_EINVAL;
    return nj_impl(h, false, true, {d_preds, d_slots, d_lengths, d_nonfinite}, B, N);
}

int pf_bionj_joins(pf_handle_t* h, const float* preds, int32_t B, int32_t N, int32_t* slots, double* lengths, uint8_t* nonfinite) {
    if (!h) return PF_EINVAL;
    return nj_impl(h, true, false, {preds, slots, lengths, nonfinite}, B, N);
}

int pf_bionj_joins_device(pf_handle_t* h, const float* d_preds, int32_t B, int32_t N, int32_t* d_slots, double* d_lengths,
                          uint8_t* d_nonfinite) {
    if (!h) return PF_EINVAL;
    return nj_impl(h, true, true, {d_preds, d_slots, d_lengths, d_nonfinite}, B, N);
}

int pf_delta(pf_handle_t* h, const float* preds, int32_t B, int32_t N, int32_t K, int64_t* pair_sum, int64_t* hist, uint8_t* nonfinite) {
    if (!h) return PF_EINVAL;
    return delta_impl(h, false, {preds, pair_sum, hist, nonfinite}, B, N, K);
}

int pf_delta_device(pf_handle_t* h, const float* d_preds, int32_t B, int32_t N, int32_t K, int64_t* d_pair_sum, int64_t* d_hist,
                    uint8_t* d_nonfinite) {
    if (!h) return PF_EINVAL;
    return delta_impl(h, true, {d_preds, d_pair_sum, d_hist, d_nonfinite}, B, N, K);
}

int pf_tree_fit(pf_handle_t* h, const float* preds, const int32_t* slots, const double* lengths, int32_t B, int32_t M, int32_t N,
                double* patristic, double* rows, int32_t* worst_j, uint8_t* status) {
    if (!h) return PF_EINVAL;
    return fit_impl(h, false, {preds, slots, lengths, patristic, rows, worst_j, status}, B, M, N);
}

int pf_tree_fit_device(pf_handle_t* h, const float* d_preds, const int32_t* d_slots, const double* d_lengths, int32_t B, int32_t M,
                       int32_t N, double* d_patristic, double* d_rows, int32_t* d_worst_j, uint8_t* d_status) {
    if (!h) return PF_EINVAL;
    return fit_impl(h, true, {d_preds, d_slots, d_lengths, d_patristic, d_rows, d_worst_j, d_status}, B, M, N);
}

int pf_tree_ols(pf_handle_t* h, const float* preds, const int32_t* slots, int32_t B, int32_t M, int32_t N, double* ols, uint8_t* status) {
    if (!h) return PF_EINVAL;
    return ols_impl(h, false, {preds, slots, ols, status}, B, M, N);
}

int pf_tree_ols_device(pf_handle_t* h, const float* d_preds, const int32_t* d_slots, int32_t B, int32_t M, int32_t N, double* d_ols,
                       uint8_t* d_status) {
    if (!h) return PF_EINVAL;
    return ols_impl(h, true, {d_preds, d_slots, d_ols, d_status}, B, M, N);
}

int pf_tree_root(pf_handle_t* h, const int32_t* slots, const double* lengths, int32_t B, int32_t M, int32_t N, double* ssq, double* pos,
                 double* mid, uint8_t* status) {
    if (!h) return PF_EINVAL;
    return root_impl(h, false, {slots, lengths, ssq, pos, mid, status}, B, M, N);
}

int pf_tree_root_device(pf_handle_t* h, const int32_t* d_slots, const double* d_lengths, int32_t B, int32_t M, int32_t N, double* d_ssq,
                        double* d_pos, double* d_mid, uint8_t* d_status) {
    if (!h) return PF_EINVAL;
    return root_impl(h, true, {d_slots, d_lengths, d_ssq, d_pos, d_mid, d_status}, B, M, N);
}

int pf_bme_nni(pf_handle_t* h, const float* preds, const int32_t* start_slots, int32_t B, int32_t N, int32_t* slots, double* lengths,
               int32_t* steps, double* tree_length, uint8_t* status) {
    if (!h) return PF_EINVAL;
    return bme_impl(h, false, false, preds, {start_slots, slots, steps, lengths, tree_length, status}, B, N);
}

int pf_bme_nni_device(pf_handle_t* h, const float* d_preds, const int32_t* d_start_slots, int32_t B, int32_t N, int32_t* d_slots,
                      double* d_lengths, int32_t* d_steps, double* d_tree_length, uint8_t* d_status) {
    if (!h) return PF_EINVAL;
    return bme_impl(h, false, true, d_preds, {d_start_slots, d_slots, d_steps, d_lengths, d_tree_length, d_status}, B, N);
}

int pf_bme_spr(pf_handle_t* h, const float* preds, const int32_t* start_slots, int32_t B, int32_t N, int32_t* slots, double* lengths,
               int32_t* steps, double* tree_length, uint8_t* status) {
    if (!h) return PF_EINVAL;
    return bme_impl(h, true, false, preds, {start_slots, slots, steps, lengths, tree_length, status}, B, N);
}

int pf_bme_spr_device(pf_handle_t* h, const float* d_preds, const int32_t* d_start_slots, int32_t B, int32_t N, int32_t* d_slots,
                      double* d_lengths, int32_t* d_steps, double* d_tree_length, uint8_t* d_status) {
    if (!h) return PF_EINVAL;
    return bme_impl(h, true, true, d_preds, {d_start_slots, d_slots, d_steps, d_lengths, d_tree_length, d_status}, B, N);
}

int pf_join_supports(pf_handle_t* h, const int32_t* ref_slots, const int32_t* rep_slots, const uint8_t* rep_flag, int32_t B, int32_t R,
                     int32_t N, int32_t* count, int64_t* transfer, int32_t* depth, uint8_t* status) {
    if (!h) return PF_EINVAL;
    return supports_impl(h, false, false, {ref_slots, rep_slots, rep_flag, count, transfer, depth, status}, B, R, N, 0);
}

int pf_join_supports_device(pf_handle_t* h, const int32_t* d_ref_slots, const int32_t* d_rep_slots, const uint8_t* d_rep_flag, int32_t B,
                            int32_t R, int32_t N, int32_t* d_count, int64_t* d_transfer, int32_t* d_depth, uint8_t* d_status) {
    if (!h) return PF_EINVAL;
    return supports_impl(h, false, true, {d_ref_slots, d_rep_slots, d_rep_flag, d_count, d_transfer, d_depth, d_status}, B, R, N, 0);
}

int pf_join_consensus(pf_handle_t* h, const int32_t* rep_slots, const double* rep_lengths, const uint8_t* rep_flag, int32_t B, int32_t R,
                      int32_t N, int32_t percent, int32_t* n_splits, int32_t* count, int32_t* size, int32_t* parent, double* split_length,
                      int32_t* leaf_parent, double* leaf_length, uint8_t* status) {
    if (!h) return PF_EINVAL;
    return consensus_impl(h, false, {rep_slots, rep_lengths, rep_flag, n_splits, count, size, parent, split_length, leaf_parent, leaf_length, status},
                          B, R, N, percent);
}

int pf_join_consensus_device(pf_handle_t* h, const int32_t* d_rep_slots, const double* d_rep_lengths, const uint8_t* d_rep_flag, int32_t B,
                             int32_t R, int32_t N, int32_t percent, int32_t* d_n_splits, int32_t* d_count, int32_t* d_size,
                             int32_t* d_parent, double* d_split_length, int32_t* d_leaf_parent, double* d_leaf_length, uint8_t* d_status) {
    if (!h) return PF_EINVAL;
    return consensus_impl(h, true, {d_rep_slots, d_rep_lengths, d_rep_flag, d_n_splits, d_count, d_size, d_parent, d_split_length, d_leaf_parent,
                                    d_leaf_length, d_status}, B, R, N, percent);
}

int pf_join_distances(pf_handle_t* h, const int32_t* slots, const double* lengths, const uint8_t* flag, int32_t B, int32_t K, int32_t N,
                      int32_t* shared, double* kf, double* wrf, uint8_t* status) {
    if (!h) return PF_EINVAL;
    return distances_impl(h, false, {slots, lengths, flag, shared, kf, wrf, status}, B, K, N);
}

int pf_join_distances_device(pf_handle_t* h, const int32_t* d_slots, const double* d_lengths, const uint8_t* d_flag, int32_t B, int32_t K,
                             int32_t N, int32_t* d_shared, double* d_kf, double* d_wrf, uint8_t* d_status) {
    if (!h) return PF_EINVAL;
    return distances_impl(h, true, {d_slots, d_lengths, d_flag, d_shared, d_kf, d_wrf, d_status}, B, K, N);
}

int pf_join_transfers(pf_handle_t* h, const int32_t* ref_slots, const int32_t* rep_slots, const uint8_t* rep_flag, int32_t B, int32_t R,
                      int32_t N, int32_t cutoff_percent, int32_t* count, int64_t* transfer, int32_t* depth, int64_t* moves, int32_t* used,
                      int32_t* capped, int32_t* branch_moves, uint8_t* status) {
    if (!h) return PF_EINVAL;
    return supports_impl(h, true, false, {ref_slots, rep_slots, rep_flag, count, transfer, depth, status, moves, used, capped, branch_moves},
                         B, R, N, cutoff_percent);
}

int pf_join_transfers_device(pf_handle_t* h, const int32_t* d_ref_slots, const int32_t* d_rep_slots, const uint8_t* d_rep_flag, int32_t B,
                             int32_t R, int32_t N, int32_t cutoff_percent, int32_t* d_count, int64_t* d_transfer, int32_t* d_depth,
                             int64_t* d_moves, int32_t* d_used, int32_t* d_capped, int32_t* d_branch_moves, uint8_t* d_status) {
    if (!h) return PF_EINVAL;
    return supports_impl(h, true, true, {d_ref_slots, d_rep_slots, d_rep_flag, d_count, d_transfer, d_depth, d_status, d_moves, d_used, d_capped,
                                     d_branch_moves}, B, R, N, cutoff_percent);
}

int pf_forward_device(pf_handle_t* h, const uint8_t* d_idx, int32_t B, int32_t N, int32_t L, float* d_out) {
    if (!h) return PF_EINVAL;
    return forward_device_impl(h, d_idx, B, N, 0, L, L, d_out);
}

int pf_forward_weighted(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, const float* w, float* out) {
    if (!h) return PF_EINVAL;
    return forward_host_impl(h, idx, B, N, 0, L, L, out, w, true);
}

int pf_forward_weighted_device(pf_handle_t* h, const uint8_t* d_idx, int32_t B, int32_t N, int32_t L, const float* d_w,
                               float* d_out) {
    if (!h) return PF_EINVAL;
    int rc = check_dims(h, B, N, L, L);
    if (rc) return rc;
    if (!d_idx || !d_w || !d_out) return fail(h, PF_EINVAL, "null buffer");
    if ((rc = check_weighted_handle(h))) return rc;
    return forward_device_impl(h, d_idx, B, N, 0, L, L, d_out, d_w);
}

int pf_forward_sites_weighted(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, const int32_t* sites,
                              const float* w, int32_t S, int32_t K, float* out) {
    if (!h) return PF_EINVAL;
    if (!sites) return fail(h, PF_EINVAL, "null buffer");
    return sites_impl(h, idx, B, N, L, sites, 0, S, K, out, w, true);
}

int pf_bootstrap_weighted(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, int32_t R, uint64_t seed,
                          float* out) {
    if (!h) return PF_EINVAL;
    return bootstrap_weighted_impl(h, idx, B, N, L, R, seed, out);
}

int pf_padded_sites(int32_t K, int32_t L) {
    const int n = pfweights::padded_sites(K, L);
    return n < 0 ? PF_EINVAL : n;
}

int pf_boot_counts(int32_t L, int32_t R, uint64_t seed, int32_t r, int32_t* sites, int32_t* counts) {
    if (L < 1 || R < 1 || r < 0 || r >= R || !sites || !counts) return PF_EINVAL;
    return pfweights::boot_counts(L, seed, r, sites, counts);
}

int pf_compress_sites(const uint8_t* idx, int32_t N, int32_t L, int32_t* first, int32_t* count) {
    if (N < 1 || L < 1 || !idx || !first || !count) return PF_EINVAL;
    std::vector<int32_t> slot;
    try { slot.resize(pfweights::compress_slots(L)); }
    catch (const std::bad_alloc&) { return PF_ENOMEM; }
    return pfweights::compress_sites(idx, N, L, first, count, slot.data());
}

int pf_site_classes(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, int32_t* srep, int32_t* ucount) {
    if (!h) return PF_EINVAL;
    if (!idx || !srep || !ucount) return fail(h, PF_EINVAL, "null buffer");
    if (B < 1 || N < 1 || L < 1) return fail(h, PF_EINVAL, "bad dimensions B=%d N=%d L=%d", B, N, L);
    size_t nidx = 0;
    if (!mul_size((size_t)B, (size_t)N, (size_t)L, &nidx)) return fail(h, PF_EINVAL, "B x N x L overflows");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t nsite = (size_t)B * L;
    int rc = h->d_idx.reserve(h, nidx);
    if (rc || (rc = h->d_map.reserve(h, (2 * nsite + B) * sizeof(int32_t)))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_idx, idx, nidx, hipMemcpyHostToDevice, h->stream));
    int32_t* d = h->d_map;
    h->cur = h->stream;
    if ((rc = launch_site_classes(h, SiteClassArgs{h->d_idx, d, d + nsite, d + 2 * nsite, N, L, h->site_dedup ? 1 : 0}, B))) return rc;
    HIPCHK(h, hipMemcpyAsync(srep, d, nsite * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(ucount, d + 2 * nsite, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PF_OK;
}

int pf_forward_site_map(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, float* out, float* map) {
    if (!h) return PF_EINVAL;
    if (!map) return fail(h, PF_EINVAL, "null buffer");
    return site_host_impl(h, idx, B, N, L, out, map, nullptr, nullptr);
}

int pf_forward_site_map_device(pf_handle_t* h, const uint8_t* d_idx, int32_t B, int32_t N, int32_t L, float* d_out, float* d_map) {
    if (!h) return PF_EINVAL;
    return site_map_device_impl(h, d_idx, B, N, L, d_out, d_map);
}

int pf_forward_site_profile(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L, float* out, float* se,
                            float* profile) {
    if (!h) return PF_EINVAL;
    if (!se || !profile) return fail(h, PF_EINVAL, "null buffer");
    return site_host_impl(h, idx, B, N, L, out, nullptr, se, profile);
}

int pf_site_moments_device(pf_handle_t* h, const float* d_map, int32_t B, int32_t P, int32_t L, float* d_se, float* d_profile) {
    if (!h) return PF_EINVAL;
    if (!d_map || !d_se || !d_profile) return fail(h, PF_EINVAL, "null buffer");
    if (B < 1 || P < 1 || L < 1) return fail(h, PF_EINVAL, "bad dimensions B=%d P=%d L=%d", B, P, L);
    size_t n = 0;
    if (!mul_size((size_t)B, (size_t)P * (size_t)L, sizeof(float), &n))
        return fail(h, PF_EINVAL, "a site map of B=%d x %d pairs x %d sites overflows the address space", B, P, L);
    HIPCHK(h, hipSetDevice(h->device));
    return launch_site_moments(h, d_map, B, P, L, d_se, d_profile);
}

int pf_forward_sharded(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t l_begin,
                       int32_t l_end, int32_t L_total, float* out) {
    if (!h) return PF_EINVAL;
    h->sharded_call = true;
    const int rc = forward_host_impl(h, idx, B, N, l_begin, l_end, L_total, out);
    h->sharded_call = false;
    return rc;
}

int pf_forward_sharded_device(pf_handle_t* h, const uint8_t* d_idx, int32_t B, int32_t N, int32_t l_begin,
                              int32_t l_end, int32_t L_total, float* d_out) {
    if (!h) return PF_EINVAL;
    h->sharded_call = true;
    const int rc = forward_device_impl(h, d_idx, B, N, l_begin, l_end, L_total, d_out);
    h->sharded_call = false;
    return rc;
}

int pf_comm_info(char* path_out, size_t path_cap, int32_t* version) {
    std::string err;
    if (!load_rccl(err)) return fail(nullptr, PF_ERCCL, "%s", err.c_str());
    if (path_out && path_cap) snprintf(path_out, path_cap, "%s", g_rccl_path.c_str());
    if (version) *version = g_rccl_version;
    return PF_OK;
}

// PF_UNIQUE_ID_BYTES = two ncclUniqueIds back to back: one per communicator (one communicator per stream).
int pf_comm_unique_id(void* id_out) {
    std::string err;
    if (!id_out) return PF_EINVAL;
    if (!load_rccl(err)) return fail(nullptr, PF_ERCCL, "%s", err.c_str());
    static_assert(PF_UNIQUE_ID_BYTES == 2 * sizeof(PfNcclId), "two ncclUniqueIds");
    for (int i = 0; i < 2; ++i) {
        int rc = g_rccl.GetUniqueId(static_cast<char*>(id_out) + i * sizeof(PfNcclId));
        if (rc != 0) return fail(nullptr, PF_ERCCL, "ncclGetUniqueId failed (%d)", rc);
    }
    return PF_OK;
}

int pf_comm_init(pf_handle_t* h, const void* unique_id, int32_t rank, int32_t world_size) {
    if (!h || world_size < 1 || rank < 0 || rank >= world_size) return PF_EINVAL;
    if (h->comm[0]) return fail(h, PF_ESTATE, "communicator already initialised");
    // rank / world are only recorded once both communicators exist: after a failed init the handle is
    // still a working single-rank engine
    if (world_size == 1 && !h->force_rccl) { h->rank = 0; h->world = 1; return PF_OK; }
    if (!unique_id) return fail(h, PF_EINVAL, "null unique id");
    std::string err;
    if (!load_rccl(err)) return fail(h, PF_ERCCL, "%s", err.c_str());
    HIPCHK(h, hipSetDevice(h->device));
    int rc0 = ensure_second_stream(h);
    if (rc0) return rc0;
    // every rank creates communicator 0, then communicator 1, in this order (ncclCommInitRank is collective)
    for (int i = 0; i < 2; ++i) {
        PfNcclId id;
        std::memcpy(id.internal, static_cast<const char*>(unique_id) + i * sizeof(PfNcclId), sizeof(PfNcclId));
        int rc = g_rccl.CommInitRank(&h->comm[i], world_size, id, rank);
        if (rc != 0) {
            h->comm[i] = nullptr;
            if (i == 1) { g_rccl.CommDestroy(h->comm[0]); h->comm[0] = nullptr; }
            return fail(h, PF_ERCCL, "ncclCommInitRank (communicator %d) failed: %s", i,
                        g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "?");
        }
    }
    h->rank = rank;
    h->world = world_size;
    return PF_OK;
}

int pf_comm_destroy(pf_handle_t* h) {
    if (!h) return PF_EINVAL;
    if (h->comm[0] || h->comm[1]) {
        hipStreamSynchronize(h->stream);
        if (h->stream2) hipStreamSynchronize(h->stream2);
        for (void*& c : h->comm) if (c) { g_rccl.CommDestroy(c); c = nullptr; }
    }
    h->world = 1; h->rank = 0;
    return PF_OK;
}

int pf_synchronize(pf_handle_t* h) {
    if (!h) return PF_EINVAL;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return check_bad_idx(h);
}

int pf_get_stream(pf_handle_t* h, void** s) {
    if (!h || !s) return PF_EINVAL;
    *s = (void*)h->stream;
    return PF_OK;
}

int pf_device_malloc(pf_handle_t* h, size_t bytes, void** out) {
    if (!h || !out) return PF_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMalloc(out, bytes ? bytes : 1));
    return PF_OK;
}
int pf_device_free(pf_handle_t* h, void* p) {
    if (!h) return PF_EINVAL;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipFree(p));
    return PF_OK;
}
int pf_memcpy_h2d(pf_handle_t* h, void* dst, const void* src, size_t bytes) {
    if (!h) return PF_EINVAL;
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PF_OK;
}
int pf_memcpy_d2h(pf_handle_t* h, void* dst, const void* src, size_t bytes) {
    if (!h) return PF_EINVAL;
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return check_bad_idx(h);
}

int pf_profile_reset(pf_handle_t* h) {
    if (!h) return PF_EINVAL;
    drain_profile(h);
    for (int i = 0; i < K_COUNT; ++i) { h->prof_n[i] = 0; h->prof_ms[i] = 0; }
    h->coll_calls = 0;
    h->rechecked = 0;
    h->nj_calls = 0;
    h->bionj_calls = 0;
    h->delta_calls = 0;
    h->fit_calls = 0;
    h->ols_calls = 0;
    h->root_calls = 0;
    h->bme_calls = 0;
    h->spr_calls = 0;
    h->sup_calls = 0;
    h->transfer_calls = 0;
    h->con_calls = 0;
    h->td_calls = 0;
    return PF_OK;
}

int pf_profile_get(pf_handle_t* h, const char* kernel, int64_t* launches, double* total_ms) {
    if (!h || !kernel) return PF_EINVAL;
    drain_profile(h);
    if (std::strcmp(kernel, "collectives") == 0) {      // always counted, no event bracketing needed
        if (launches) *launches = h->coll_calls;
        if (total_ms) *total_ms = 0.0;
        return PF_OK;
    }
    if (std::strcmp(kernel, "rechecked") == 0) {        // alignments the range re-check sent to the float64 kernels
        if (launches) *launches = h->rechecked;
        if (total_ms) *total_ms = 0.0;
        return PF_OK;
    }
    if (std::strcmp(kernel, "nj_joins") == 0) {         // pf_nj_joins / pf_nj_joins_device calls
        if (launches) *launches = h->nj_calls;
        if (total_ms) *total_ms = 0.0;
        return PF_OK;
    }
    if (std::strcmp(kernel, "bionj_joins") == 0) {      // pf_bionj_joins / pf_bionj_joins_device calls
        if (launches) *launches = h->bionj_calls;
        if (total_ms) *total_ms = 0.0;
        return PF_OK;
    }
    if (std::strcmp(kernel, "delta") == 0) {            // pf_delta / pf_delta_device calls
        if (launches) *launches = h->delta_calls;
        if (total_ms) *total_ms = 0.0;
        return PF_OK;
    }
    if (std::strcmp(kernel, "tree_fit") == 0) {         // pf_tree_fit / pf_tree_fit_device calls
        if (launches) *launches = h->fit_calls;
        if (total_ms) *total_ms = 0.0;
        return PF_OK;
    }
    if (std::strcmp(kernel, "tree_ols") == 0) {         // pf_tree_ols / pf_tree_ols_device calls
        if (launches) *launches = h->ols_calls;
        if (total_ms) *total_ms = 0.0;
        return PF_OK;
    }
    if (std::strcmp(kernel, "tree_root") == 0) {        // pf_tree_root / pf_tree_root_device calls
        if (launches) *launches = h->root_calls;
        if (total_ms) *total_ms = 0.0;
        return PF_OK;
    }
    if (std::strcmp(kernel, "bme_nni") == 0) {          // pf_bme_nni / pf_bme_nni_device calls
        if (launches) *launches = h->bme_calls;
        if (total_ms) *total_ms = 0.0;
        return PF_OK;
    }
    if (std::strcmp(kernel, "bme_spr") == 0) {          // pf_bme_spr / pf_bme_spr_device calls
        if (launches) *launches = h->spr_calls;
        if (total_ms) *total_ms = 0.0;
        return PF_OK;
    }
    if (std::strcmp(kernel, "join_supports") == 0) {    // pf_join_supports / pf_join_supports_device calls
        if (launches) *launches = h->sup_calls;
        if (total_ms) *total_ms = 0.0;
        return PF_OK;
    }
    if (std::strcmp(kernel, "join_transfers") == 0) {   // pf_join_transfers / pf_join_transfers_device calls
        if (launches) *launches = h->transfer_calls;
        if (total_ms) *total_ms = 0.0;
        return PF_OK;
    }
    if (std::strcmp(kernel, "join_distances") == 0) {   // pf_join_distances / pf_join_distances_device calls
        if (launches) *launches = h->td_calls;
        if (total_ms) *total_ms = 0.0;
        return PF_OK;
    }
    if (std::strcmp(kernel, "join_consensus") == 0) {   // pf_join_consensus / pf_join_consensus_device calls
        if (launches) *launches = h->con_calls;
        if (total_ms) *total_ms = 0.0;
        return PF_OK;
    }
    for (int i = 0; i < K_COUNT; ++i)
        if (std::strcmp(kernel, KNAMES[i]) == 0) {
            if (launches) *launches = h->prof_n[i];
            if (total_ms) *total_ms = h->prof_ms[i];
            return PF_OK;
        }
    return fail(h, PF_EINVAL, "unknown kernel '%s'", kernel);
}

int64_t pf_debug_read(pf_handle_t* h, const char* name, float* dst, int64_t cap) {
    if (!h || !name) return PF_EINVAL;
    if (std::strcmp(name, "phase_prof") == 0) {
        if (!h->phase_prof) return fail(h, PF_ESTATE, "phase_prof not enabled");
        unsigned long long v[8];
        hipStreamSynchronize(h->stream);
        if (hipMemcpy(v, h->phase_prof, 64, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, PF_EHIP, "phase_prof copy");
        for (int i = 0; i < 8 && i < cap; ++i) dst[i] = (float)((double)v[i] * 1e-6);   // mega-cycles
        return 8;
    }
    if (std::strcmp(name, "f16_ranges") == 0) {       // [checkpoint inside the fp16 operand ranges, bound of the column |v|],
        // and for a caller with room for six: [hidden, row-mix base * 64, weights, out_proj biases], for seven: [the largest
        // out_proj row sum] (check_f16_ranges)
        if (dst && cap > 0) dst[0] = h->f16_ok ? 1.f : 0.f;
        if (dst && cap > 1) dst[1] = (float)h->f16_vmax_col;
        if (!dst || cap < 6) return 2;
        const int n = cap < 7 ? 6 : 7;
        for (int i = 0; i + 2 < n; ++i) dst[2 + i] = (float)h->f16_bounds[i];
        return n;
    }
    auto it = h->taps.find(name);
    if (it == h->taps.end()) return fail(h, PF_ESTATE, "no tap '%s' (set debug_keep=1 and run a forward)", name);
    const int64_t n = (int64_t)it->second.size();
    if (dst) std::memcpy(dst, it->second.data(), (size_t)std::min(n, cap) * sizeof(float));
    return n;
}

int pf_device_info(pf_handle_t* h, char* name_out, size_t name_cap, int32_t* cu_count, uint64_t* hbm_bytes) {
    if (!h) return PF_EINVAL;
    if (name_out && name_cap) {
        // (the pool's boxes report an empty marketing name: fall back to hipDeviceGetName, then to the architecture)
        char nm[256] = {0};
        snprintf(nm, sizeof nm, "%s", h->prop.name);
        if (!nm[0] && hipDeviceGetName(nm, (int)sizeof nm, h->device) != hipSuccess) nm[0] = 0;
        if (!nm[0]) snprintf(nm, sizeof nm, "AMD GPU");
        snprintf(name_out, name_cap, "%s (%s)", nm, h->prop.gcnArchName);
    }
    if (cu_count) *cu_count = h->prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = h->prop.totalGlobalMem;
    return PF_OK;
}

int pf_device_pci(pf_handle_t* h, int32_t* domain, int32_t* bus, int32_t* device) {
    if (!h) return PF_EINVAL;
    if (domain) *domain = h->prop.pciDomainID;
    if (bus) *bus = h->prop.pciBusID;
    if (device) *device = h->prop.pciDeviceID;
    return PF_OK;
}

// Single-GPU emulation of the site-sharded forward ("fake backend" for tests): the alignment's
// sites are split into `nshards` ranges exactly as phyloformer_amd/dist.py::site_range does, every
// non-empty shard gets its own workspace, and the schedule of a real rank runs over all of them in rank order
// on the main stream, the collectives replaced by device-side sums in rank order.  idx: host uint8 [B][N][L].
int pf_forward_shards_emulated(pf_handle_t* h, const uint8_t* idx, int32_t B, int32_t N, int32_t L,
                               int32_t nshards, float* out) {
    if (!h) return PF_EINVAL;
    int rc = check_dims(h, B, N, L, L);
    if (rc) return rc;
    if (nshards < 1 || nshards > 64 || !idx || !out) return fail(h, PF_EINVAL, "bad shard count or null buffer");
    HIPCHK(h, hipSetDevice(h->device));
    if (const F64Path* f = f64_path_of(h, N, L)) return forward_shards_emulated_f64(h, *f, idx, B, N, L, nshards, out);
    if ((rc = ensure_pairs(h, N))) return rc;
    const int P = N * (N - 1) / 2;
    ShardStage stage(h);
    if ((rc = stage.upload(idx, B, N, L, nshards))) return rc;
    std::vector<ShardRun> runs;
    for (const ShardStage::Shard& s : stage.shards) {
        ShardRun r = shard_run(h, s.d_idx, nullptr, B, N, s.Lloc, L);
        auto list = workspace_list(h, r.w, B, P, s.Lloc);
        char* ws = (char*)stage.alloc(pfspan::measure(list, 256));
        r.d_out = (float*)stage.alloc((size_t)B * P * sizeof(float));
        if (!ws || !r.d_out) return fail(h, PF_ENOMEM, "shard workspace allocation failed");
        pfspan::carve(ws, list, 256);
        runs.push_back(r);
    }
    // the "all-reduced" buffer every emulated rank reads
    float* total = (float*)stage.alloc((size_t)B * P * SROW * sizeof(float));
    if (!total) return fail(h, PF_ENOMEM, "shard sum buffer");
    auto reduce = [&](bool site_sums) -> int {
        const size_t count = (size_t)B * P * (site_sums ? 1 : SROW);
        for (ShardRun& r : runs)                                   // every rank reduces its own tiles first
            if (!site_sums && (rc = launch_rowsum(h, r, &r.rs))) return rc;
        hipMemsetAsync(total, 0, count * sizeof(float), h->stream);
        for (ShardRun& r : runs) {
            hipLaunchKernelGGL(k_accumulate, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream,
                               total, site_sums ? r.d_out : r.w.srow, count);
            r.rs = RowStats{total, 1, 0};
        }
        return PF_OK;
    };
    rc = schedule(h, runs.data(), runs.size(), reduce);
    if (!rc && (hipMemcpyAsync(out, total, (size_t)B * P * sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
                hipStreamSynchronize(h->stream) != hipSuccess))
        rc = fail(h, PF_EHIP, "result copy failed");
    return rc;
}

// Hardware-layout self test (see k_selftest); out must hold 2304 floats.
int pf_selftest(pf_handle_t* h, float* out) {
    if (!h || !out) return PF_EINVAL;
    float* d = nullptr;
    HIPCHK(h, hipMalloc((void**)&d, 2304 * sizeof(float)));
    hipLaunchKernelGGL(k_selftest, dim3(1), dim3(64), 0, h->stream, d);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, d, 2304 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    hipFree(d);
    return PF_OK;
}

// ---- softmax MultiHeadAttention (kernels in pf_mha.hip.h) -------------------
struct pf_mha {
    pf_handle* h = nullptr;
    float* wfrag = nullptr;   // MHA_WTOTAL fragments: Wq, Wk, Wv, Wo as hi / lo
    float* bias = nullptr;    // [4][64]
    std::vector<DeviceBuffer*> buffers;
    Buffer<char> ws{buffers};                     // pfspan::mha_arrays
    Buffer<float> d_x{buffers}, d_y{buffers};     // staging for the host-buffer entry point
};

int pf_mha_create(pf_handle_t* h, const pf_mha_weights_t* w, pf_mha_t** out) {
    if (!h || !w || !out) return PF_EINVAL;
    if (w->n_heads != MHA_H || w->embed_dim != E)
        return fail(h, PF_EINVAL, "softmax attention kernels are specialised for embed_dim 64 / 4 heads, got %d / %d",
                    w->embed_dim, w->n_heads);
    const float* ws[4] = {w->wq, w->wk, w->wv, w->wo};
    const float* bs[4] = {w->bq, w->bk, w->bv, w->bo};
    std::vector<uint16_t> img((size_t)MHA_WTOTAL * 8);
    std::vector<float> bias(4 * E);
    for (int i = 0; i < 4; ++i) {
        if (!ws[i] || !bs[i]) return fail(h, PF_EINVAL, "pf_mha_create: NULL weight pointer");
        std::copy(bs[i], bs[i] + E, bias.begin() + i * E);
    }
    pack_frags(w->wq, E, E, E, img.data());
    pack_frags(w->wk, E, E, E, img.data() + (size_t)MHA_OFF_WK * 8);
    pack_frags(w->wv, E, E, E, img.data() + (size_t)MHA_OFF_WV * 8);
    pack_frags(w->wo, E, E, E, img.data() + (size_t)MHA_OFF_WO * 8);
    HIPCHK(h, hipSetDevice(h->device));
    pf_mha* m = new pf_mha();
    m->h = h;
    void* p = nullptr;
    if (hipMalloc(&p, img.size() * 2) != hipSuccess) { delete m; return fail(h, PF_ENOMEM, "pf_mha_create: hipMalloc failed"); }
    m->wfrag = (float*)p;
    if (hipMalloc(&p, bias.size() * 4) != hipSuccess) { hipFree(m->wfrag); delete m; return fail(h, PF_ENOMEM, "pf_mha_create: hipMalloc failed"); }
    m->bias = (float*)p;
    if (hipMemcpy(m->wfrag, img.data(), img.size() * 2, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(m->bias, bias.data(), bias.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(m->wfrag); hipFree(m->bias); delete m;
        return fail(h, PF_EHIP, "pf_mha_create: weight upload failed");
    }
    *out = m;
    return PF_OK;
}

int pf_mha_destroy(pf_mha_t* m) {
    if (!m) return PF_OK;
    hipSetDevice(m->h->device);
    hipStreamSynchronize(m->h->stream);
    hipFree(m->wfrag); hipFree(m->bias);
    for (DeviceBuffer* b : m->buffers) b->release();
    delete m;
    return PF_OK;
}

int pf_mha_forward_device(pf_mha_t* m, const float* d_x, int32_t B, int32_t R, int32_t C, float* d_y) {
    if (!m || !d_x || !d_y) return PF_EINVAL;
    pf_handle* h = m->h;
    if (B < 1 || R < 1 || C < 1) return fail(h, PF_EINVAL, "pf_mha_forward: need B, R, C >= 1, got %d, %d, %d", B, R, C);
    const int64_t rows64 = (int64_t)B * R;
    const int ntiles = (C + 31) / 32;
    if (rows64 * MHA_H * ((ntiles + 3) / 4) > 0x7fffffffLL || rows64 * ntiles > 0x7fffffffLL)
        return fail(h, PF_EINVAL, "pf_mha_forward: B*R*C too large for one launch");
    const int rows = (int)rows64;
    HIPCHK(h, hipSetDevice(h->device));
    MhaArgs a;
    auto list = [&](auto& v) { pfspan::mha_arrays(v, a.qp, a.kp, a.vp, a.att, (size_t)rows, (size_t)MHA_H, (size_t)ntiles, (size_t)C, (size_t)E); };
    if (const int rc = m->ws.reserve(h, pfspan::measure(list, 256))) return rc;
    pfspan::carve(m->ws, list, 256);
    a.x = d_x; a.y = d_y;
    a.wfrag = (const frag_t*)m->wfrag;
    a.bias = m->bias;
    a.rows = rows; a.C = C; a.ntiles = ntiles;
    a.qscale = (float)(1.4426950408889634 / std::sqrt((double)MHA_D));
    const int cus = h->prop.multiProcessorCount > 0 ? h->prop.multiProcessorCount : 256;
    const int lin_tiles = rows * ntiles;
    const int g1 = std::max(1, std::min((lin_tiles + 3) / 4, cus * 3));
    {
        ProfScope ps(h, K_MHA_QKV);
        launch_mha_qkv(h->stream, (unsigned)g1, a);
    }
    HIPCHK(h, hipGetLastError());
    {
        ProfScope ps(h, K_MHA_ATTN);
        launch_mha_attn(h->stream, (unsigned)(rows * MHA_H * ((ntiles + 3) / 4)), a);
    }
    HIPCHK(h, hipGetLastError());
    const int64_t out_tiles = ((int64_t)rows * C + 31) / 32;
    const int g3 = (int)std::max<int64_t>(1, std::min<int64_t>((out_tiles + 3) / 4, cus * 8));
    {
        ProfScope ps(h, K_MHA_OUT);
        launch_mha_out(h->stream, (unsigned)g3, a);
    }
    HIPCHK(h, hipGetLastError());
    return PF_OK;
}

int pf_mha_forward(pf_mha_t* m, const float* x, int32_t B, int32_t R, int32_t C, float* y) {
    if (!m || !x || !y) return PF_EINVAL;
    pf_handle* h = m->h;
    if (B < 1 || R < 1 || C < 1) return fail(h, PF_EINVAL, "pf_mha_forward: need B, R, C >= 1, got %d, %d, %d", B, R, C);
    HIPCHK(h, hipSetDevice(h->device));
    const size_t bytes = (size_t)B * R * C * E * 4;
    int rc = m->d_x.reserve(h, bytes);
    if (rc || (rc = m->d_y.reserve(h, bytes))) return rc;
    HIPCHK(h, hipMemcpyAsync(m->d_x, x, bytes, hipMemcpyHostToDevice, h->stream));
    if ((rc = pf_mha_forward_device(m, m->d_x, B, R, C, m->d_y))) return rc;
    HIPCHK(h, hipMemcpyAsync(y, m->d_y, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PF_OK;
}

}  // extern "C"
