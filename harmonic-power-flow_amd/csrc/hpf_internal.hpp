// Internal declarations shared by the translation units of libhpf.so (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <stdint.h>

#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/hpf.h"
#include "hpf_assembly.hpp"
#include "hpf_devmem.hpp"
#include "hpf_switches.hpp"

namespace hpf {

// device blocks come from hipMalloc (hpf_devmem.hpp: the one place that allocates and frees them)
struct HipBackend {
    static constexpr int oom = (int)hipErrorOutOfMemory;
    static int alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
    static int free(void* p) { return (int)hipFree(p); }
    static int copy_in(void* dst, const void* src, size_t bytes) { return (int)hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
};
using DevMem = DevOwner<HipBackend>;

// One sweep accumulator of a handle (hpf_accum.hpp): everything is allocated from `mem` while open and goes in one clear().
struct Accum {
    explicit Accum(int* detail) : mem(detail) {}
    bool open = false;
    double* f = nullptr;              // [nf] max | sum | sum of squares of every quantity (AccumSlot)
    int* arg = nullptr;               // [narg] scenario id of every maximum (-1: nothing added)
    uint32_t* over = nullptr;         // [nover] scenarios over the limit (and whatever the feature keeps behind them)
    long long* cnt = nullptr;         // [3] added, skipped, deferred
    double* limit = nullptr;          // the per-owner limits
    size_t nf = 0, narg = 0, nover = 0;
    DevMem mem;                       // (last: it goes first)
};

// form of the 2x2 algebra of the all-linear subtrees in a block-tree Newton step (Tree::lin_form, decided by the planner)
enum LinForm {
    LIN_ROOTS = 0,                    // uncontracted tree: one thread per (linear root, harmonic) walks its subtree (k_lin_factor / k_lin_back)
    LIN_BUNDLE,                       // one-round-trip bundles, Tree::lin_np items per thread (k_lin_bundle_factor / _back)
    LIN_TREE,                         // bundles of whole subtrees, every height in one launch (k_lin_tree_factor / _back)
    LIN_LEVELS                        // one launch per height (k_lin_level_factor / _back)
};

enum { T_MISMATCH = 0, T_JACOBIAN = 1, T_SOLVE = 2, T_UPDATE = 3, T_BACK = 4, T_GJ = 5, T_GJ_DEV = 6, T_RESID = 7, T_COUNT = 8 };

struct TimedSpan {
    int which;
    hipEvent_t e0, e1;
};

// back-sweep tree walk: at most WALK_LISTS subtree lists (x 32 scenarios: one workgroup per CU), an LDS ring of the x of the last
// WALK_SLOTS buses a workgroup walked
#ifndef HPF_WALK_SLOTS
#define HPF_WALK_SLOTS 32             // (a build flag for tests of the ring at another size)
#endif
constexpr int WALK_LISTS = 8, WALK_SLOTS = HPF_WALK_SLOTS;
static_assert(WALK_SLOTS >= 2, "the walk's ring holds at least the previous bus");
// back-sweep tail: LDS slots of a family's store of x (16 scenarios each); the children of a bus that gets none read its x from HBM
constexpr int TAIL_SLOTS = 2;

// Feeder-tree description for the BLOCK_TREE solver (host copies + device copies).
struct Tree {
    int n_levels = 0;                 // elimination levels (by height, leaves first)
    int n_depths = 0;                 // back-substitution levels (by depth, root first)
    std::vector<int> parent;          // [n], -1 for the root (bus 0)
    std::vector<int> lvl_ptr;         // [n_levels+1] into lvl_nodes
    std::vector<int> lvl_nodes;       // nodes grouped by height
    std::vector<int> dep_ptr;         // [n_depths+1] into dep_nodes
    std::vector<int> dep_nodes;       // nodes grouped by depth
    std::vector<int> child_ptr;       // [n+1]
    std::vector<int> child;           // children lists: all-linear-subtree children first, then dense children
    std::vector<int> child_mid;       // [n] end of the linear children inside a node's child list
    std::vector<int> lin;             // [n] 1: the whole subtree of the bus is linear -> harmonic-diagonal 2x2 algebra
    std::vector<int> lin_ptr;         // [n_lin_roots+1] into lin_post
    std::vector<int> lin_post;        // post-order node lists of the maximal linear subtrees
    std::vector<int> all_ptr, all_post;   // the whole tree as one post-order list (fundamental power flow)
    int n_lin_roots = 0;
    int n_dense = 0;
    int* d_parent = nullptr;
    int* d_lvl_nodes = nullptr;
    int* d_dep_nodes = nullptr;
    int* d_child_ptr = nullptr;
    int* d_child = nullptr;
    int* d_e_up = nullptr;            // [n] CSR position of entry (i, parent(i))
    int* d_e_dn = nullptr;            // [n] CSR position of entry (parent(i), i)
    int* d_child_mid = nullptr;
    int* d_lin = nullptr;
    int* d_lin_ptr = nullptr;
    int* d_lin_post = nullptr;
    int* d_all_ptr = nullptr;
    int* d_all_post = nullptr;
    int* d_fdesc = nullptr;           // [n_dense][16] node records of the multi-wave factor kernel, elimination-level order:
                                      //   k, parent, diag entry, device, e_dn, e_up, lin child begin, count, dense child begin,
                                      //   count, first four dense children (everything a block needs behind ONE scalar load)
    int* d_child3 = nullptr;          // [n-1][4] per child-list position: child, e_dn[child], e_up[child], 0
    int* d_bdesc = nullptr;           // [n_dense][4] (k, dense parent, constant-inverse slot + 1, 0) in back-substitution (depth) order
    // contraction of pass-through buses (linear bus, exactly one dense child): eliminated in 2x2-per-harmonic algebra before
    // the dense levels; `parent` stays the network parent, the dense tree links a chain's bottom bus to the chain's top parent
    int n_chains = 0;
    std::vector<int> chain_ptr, chain_nodes, chain_ch;   // chains bottom-up: nodes k1..kt, ch = the dense bus below k1
    int* d_dchild = nullptr;          // dense children lists of the dense buses (through chains), indexed by the node records
    int* d_chain_ptr = nullptr;
    int* d_chain_nodes = nullptr;
    int* d_chain_ch = nullptr;
    // constant-inverse leaves (contracted tree only): nonlinear buses without dense children.  In rectangular coordinates their
    // block is  R(y_kk I - Y_N - series terms of the linear neighbourhood)  + a 2x2 state-dependent term at the fundamental, so
    // the inverse of the harmonic part and its borders are computed ONCE per model (host, complex) and kept as a b x b image
    // [c0 Lr; Lc Ahh^-1] in accumulator-tile layout; the device adds the rank-2 term  [I; Lc] (c0 + D)^-1 [I Lr]
    // level-parallel kernels of the 2x2 algebra (contracted tree): all-linear-subtree buses grouped by their height inside the
    // subtree, one record of 8 ints per bus (k, diagonal entry, parent, e_up, e_dn, first child position, children, 0); chains:
    // 8 ints per chain (ch, e_dn[ch], e_up[ch], first node record, nodes, 0, 0, 0) and the same node records, bottom-up
    int n_lin_heights = 0;
    std::vector<int> lh_ptr;          // [n_lin_heights+1] into the records
    int* d_lrec = nullptr;
    // ... and the same records once more, grouped into bundles of whole subtrees (k_lin_tree_factor / k_lin_tree_back: one launch
    // for all heights): records sorted by (bundle, height), lb_ptr [n_lin_bundles][n_lin_heights + 1] offsets into them
    // ... and for the one-round-trip kernels (k_lin_bundle_factor / _back): bundles of at most 256 * lin_np items (bus, harmonic),
    // records with cbeg = first child slot, d_lb2x[record] = (own slot | -1, local index of the parent | -1)
    int n_lin_bundles2 = 0, lin_np = 0;
    int lin_maxunit = 0;              // buses of the largest unit (a chain's hanging subtrees, or a free subtree) the bundles are sized by
    int* d_lb2rec = nullptr;
    int* d_lb2x = nullptr;
    int* d_lb2ptr = nullptr;
    int chains_bundled = 0;           // the contracted chains ride in the bundle launches (d_lb2cptr [bundle + 1] into d_lb2clist: chain ids)
    int* d_lb2cptr = nullptr;
    int* d_lb2clist = nullptr;
    int n_lin_bundles = 0;
    LinForm lin_form = LIN_ROOTS;
    bool chain_launches = false;      // the contracted chains get their own launches (k_chain_factor2 / k_chain_back2)
    int* d_lbrec = nullptr;
    int* d_lbptr = nullptr;
    int* d_crec = nullptr;            // chain headers
    int* d_cnode = nullptr;           // chain node records
    int n_all_heights = 0;            // the whole tree by height (fundamental power flow)
    std::vector<int> ah_ptr;
    int* d_arec = nullptr;
    std::vector<int> lvl_all_leaf;    // [n_levels] 1: every bus of the elimination level is a constant-inverse leaf
    std::vector<int> toff_tab;        // [b][b] offset of (row, col) of a block in a tile image (TileIO<B>::off), -1: not stored
    std::vector<char> plain_gj;       // [n] 1: dense bus on the plain Gauss-Jordan path (its inverse S_k^-1 is in its inverse slot after a sweep)
    int n_cleaf = 0;
    double* d_Minv = nullptr;         // [n_cleaf][NT*NT*256]
    // lazy leaves: constant-inverse leaves directly under their dense parent never write their Schur complement; the parent
    // rebuilds the sum from per-model images and the leaves' 2x2 cores (k_factor_q, "lazy" phase)
    int n_lazy_parents = 0, n_lazy_leaves = 0;
    int n_lazy_level0 = 0;            // the first n_lazy_level0 buses of elimination level 0 are lazy leaves (k_leaf_batch)
    std::vector<int> lvl_nbatch;      // [n_levels] super-leaves of a level whose parent rebuilds their Schur complement: they come first
                                      // in the level's records and go through k_sleaf_batch (16 scenarios per workgroup)
    std::vector<int> dep_nleaf;       // [n_depths] constant-inverse leaves of a back-sweep depth (they come first in the depth's records)
    std::vector<int> dep_nskip;       // [n_depths] leaves + batched super-leaves of a depth: k_back_q starts behind them
    int census[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // hpf_tree_census
    std::vector<int> bsleaf_ptr;      // back sweep of the bordered buses in groups by nesting order (nested ones first): offsets into d_bsleaf
    int n_bsleaf = 0;
    int* d_bsleaf = nullptr;          // [n_bsleaf][8] back-sweep records of the super-leaves (k_sleaf_back_batch)
    double* d_sbimg = nullptr;        // [n_bsleaf][SleafImg<B>::SZ] their [0 0; 0 Ahh^-1] images (+ Qb rows) and Pb in MFMA A-operand layout
    std::vector<int> bsl_dep_ptr, bleaf_dep_ptr;   // [n_depths + 1] the same records by back-sweep depth (d_bsleaf_dep: depth order; d_bleaf is in depth order): k_level_back
    int* d_bsleaf_dep = nullptr;
    int n_bleaf = 0;
    int* d_bleaf = nullptr;           // [n_bleaf][4] back-sweep records of ALL constant-inverse leaves: one k_leaf_back_batch launch after the last depth
    double* d_lbimg = nullptr;        // [leaf slot][LeafBatchImg::SZ]: the leaf images in MFMA A-operand layout (16 scenarios per workgroup)
    int* d_lzrec = nullptr;           // [n_lazy_parents][8]: image offset (doubles), L, leaf ids[4] (-1: none), 0, 0
    double* d_lzimg = nullptr;        // per parent: sum of constant parts (tile layout) | A operands [pair][tr][64] | row factors [pair][tc][2][64]
    // compress steps on the Gauss-Jordan skeleton (contracted tree, HPF_COMPRESS != 0): bus v = comp_v[i] is eliminated BEFORE its
    // pending child c = comp_c[i] (its tallest dense child, alone on v's critical path); c then hangs under v's parent p with a dense
    // coupling pair, the elimination levels / back-sweep depths are the longest paths of the new dependencies
    int n_comp = 0;
    std::vector<int> comp_v, comp_c;
    int* d_comp_child = nullptr;      // [n_comp] c of compress step i (k_back_q: x_v needs x_c)
    // back-sweep tree walk (k_back_walk, blocks of 52, leaf batching on): the Gauss-Jordan buses the back sweep's depth launches would take,
    // as work lists of Tree::d_bdesc records -- list 0 the trunk (the top walk_depth depths, one launch), lists 1..walk_lists the subtrees
    // below it (one launch), each root-first, with the LDS ring slots of the x of its parent and of its pending child c (-1: from HBM)
    int walk_lists = 0;               // branch lists (0: no schedule)
    int walk_depth = 0;               // depths in the trunk
    std::vector<int> walk_ptr;        // [walk_lists + 2] list l: records walk_ptr[l] .. walk_ptr[l + 1]
    std::vector<int> walk_rec;        // [][4] the d_bdesc records
    std::vector<int> walk_slot;       // [][2] ring slot of x_parent, of x_c
    int* d_walk_ptr = nullptr;
    int* d_walk_rec = nullptr;
    int* d_walk_slot = nullptr;
    // back-sweep tail (k_back_tail): the records of d_bsleaf and d_bleaf in families -- a batched bus whose dense parent is not batched (a bordered
    // bus or a leaf under a Gauss-Jordan bus), then its nested bordered buses and the leaves below any of them, every member after its parent;
    // families longest first.  One record per member: kind (0 bordered, 1 leaf), index of its record in d_bsleaf / d_bleaf, LDS slot of its
    // parent's x (-1: from HBM, an earlier launch wrote it; -2: from HBM, the family's workgroup wrote it), LDS slot its own x goes to (-1: none of its family reads it from LDS)
    int n_tail_fam = 0;
    std::vector<int> tail_ptr;        // [n_tail_fam + 1] family f: members tail_ptr[f] .. tail_ptr[f + 1]
    std::vector<int> tail_rec;        // [][4]
    int* d_tail_ptr = nullptr;
    int* d_tail_rec = nullptr;
    double plan_ms = 0.0;             // host time of tree_build_into up to the uploads (all planning, the back-sweep batch records included)
    double flops_per_solve = 0.0;     // factor sweep + back sweep
    double flops_factor = 0.0;        // factor sweep only (k_tree_factor, all levels)
    double bytes_back = 0.0;          // algorithmic HBM bytes of the dense back sweep, one scenario and step
    double bytes_factor = 0.0;        // algorithmic HBM bytes of the factor sweep, one scenario and step (see hpf_solve_bytes)
    double flops_gj = 0.0, bytes_gj = 0.0;   // the share of the buses that go through the general kernel k_factor_q<B, false>
    int n_gj_launches = 0;            // launches of that kernel per sweep (and scenario group)
};

}  // namespace hpf

struct hpf_handle {
    hpf::Switches sw;                 // build switches (hpf_switches.hpp), parsed once by hpf_create
    hpf::Model M{};                   // device pointers
    int n = 0, m = 0, c = 0, Hn = 0, nnz = 0, n_dev = 0, coupled = 0, solver = 0, device = 0;
    int S_max = 0, S = 0;
    int S_alloc = 0;                  // scenario slots allocated = S_max (+ 1 + m_border virtual slots of the bordered Newton step)
    // meshed networks on the block-tree path (hpf_block.hip, "bordered Newton step"): BFS spanning tree + loop-closing lines
    int n_ties = 0, n_tb = 0, m_border = 0;      // tie lines, their distinct endpoint buses, border unknowns = n_tb * 2 Hn
    int *d_tb_bus = nullptr;          // [n_tb] endpoint buses
    int *d_tb_ptr = nullptr;          // [n_tb + 1] into d_tb_adj
    int *d_tb_adj = nullptr;          // per (endpoint i, tie (i,j)): j, CSR entry (i,j), 0
    double *d_bM = nullptr, *d_brhs = nullptr;   // border system (m x m column-major, m)
    int *d_bipiv = nullptr, *d_binfo = nullptr;
    double *d_bM0 = nullptr, *d_brhs0 = nullptr;   // kept copy of the border system (residual check of the unpivoted LU) | copy of its right-hand side + 2 check words
    // factor-once form of the bordered step (tree_sel_build / tree_sel_run, hpf_block.hip): the tree is swept ONCE per Newton step and scenario
    // for y = J_t^-1 f; the border matrix comes from a selected inversion over P = the union of the endpoints' root paths, whose buses the planner
    // keeps as plain Gauss-Jordan buses (sel_forced) so that S_k^-1 sits in their inverse slot
    bool mesh_sel = false;
    std::vector<char> sel_forced;     // [n] 1: bus on a root path of a tie endpoint (empty: not used)
    std::vector<int> tb_bus_host;     // [n_tb] endpoint buses (host copy of d_tb_bus)
    int sel_nP = 0, sel_npairs = 0, sel_R = 0;
    int *d_sel_P = nullptr;           // [nP][4]: bus, index of its parent in P (-1: root), CSR entries (bus, parent), (parent, bus)
    int *d_sel_pidx = nullptr;        // [n] index in P or -1
    int *d_sel_toff = nullptr;        // [b][b] offset of (row, col) in a tile image of the inverse slot
    double *d_sel_S = nullptr, *d_sel_Z = nullptr, *d_sel_Up = nullptr;   // [nP][b][b] S^-1, S^-1 A(k, parent), S_parent^-1 A(parent, k): dense, row-major
    double *d_sel_W = nullptr;        // [npairs][b][b] forward blocks W[k, t]
    double *d_sel_X = nullptr;        // [nP][n_tb][b][b] (J_t^-1 E_T) restricted to P
    double *d_sel_tie = nullptr;      // [2 n_ties][Hn][4] the ties' coupling blocks of the current state
    void *d_sel_jobs = nullptr;       // BlkJob list: forward by height, back by depth
    std::vector<size_t> sel_fwd_beg, sel_back_beg, sel_hl_ptr;
    int *d_sel_hl = nullptr, *d_sel_slot = nullptr, *d_sel_cptr = nullptr, *d_sel_clist = nullptr;   // P by height | endpoint number | children in P
    double *d_sel_dw = nullptr;       // [nP][b] corrections of the forward vectors
    int sel_cap = 1;                  // scenarios whose selected inversion / border solve run as one batch (every d_sel_* / d_bB buffer holds that many)
    double *d_sel_bM = nullptr, *d_sel_rhs = nullptr, *d_sel_g = nullptr;   // per batch position: border matrix (column-major, untouched by the solve), Q^T y, solution g
    unsigned long long* d_sel_res = nullptr;   // [sel_cap][2] residual check words (k_border_check)
    int* d_sel_info = nullptr;        // [sel_cap] weak / zero pivot of the block Gauss-Jordan solve, info of the unpivoted LU
    std::vector<unsigned long long> sel_res_host;
    std::vector<int> sel_info_host;
    bool border_gj = false;           // border system by block Gauss-Jordan on the b x b grid (n_tb <= HPF_BORDER_GJ, default 96) instead of rocSOLVER's LU
    double *d_bB = nullptr;           // [n_tb][n_tb + 1][b][b] the border system in block layout, right-hand side in block column n_tb
    void *d_bgj_jobs = nullptr;       // its block-product jobs: per step the row scaling, then the elimination
    std::vector<size_t> bgj_beg;
    int border_pivoting = 0;          // option "border_pivoting": 1 = every border system through the pivoted LU (A/B, tests)
    int border_repivots = 0;          // border systems that went through the pivoted LU after the residual check
    std::vector<int> host_act;        // the slot list as the host last saw it (the bordered step walks the running scenarios)
    int N = 0, Nc = 0, Nf = 0;
    bool loads_set = false, state_set = false, mismatch_valid = false;
    int last_detail = 0;
    const char* plan_path = nullptr;  // hpf_tree_plan: file the planning run writes (instead of env HPF_TREE_DUMP) ...
    bool plan_only = false;           // ... and it stops before the uploads
    bool plan_written = false;
    int gj_mode = 1;                  // (initially sw.gj_mode) BLOCK_TREE block inversion: 0 pivoted wave Gauss-Jordan (VALU, uncontracted tree), 1 MFMA static 4x4 blocks, NT waves per bus (hpf_quad.hpp)
    double piv_limit = 1e10;          // static pivot order: amplification of a 4x4 pivot block's inverse beyond which a scenario is repeated with partial pivoting

    // model (device)
    int* d_rowrec = nullptr;          // [n][8] row records of the mismatch kernel (Model::rowrec)
    int *d_rowptr = nullptr, *d_col = nullptr, *d_diag = nullptr, *d_erow = nullptr, *d_dev = nullptr;
    hpf::cplx *d_Y = nullptr, *d_YN = nullptr, *d_IN = nullptr, *d_YNt = nullptr;
    // per-scenario state (device)
    double *d_P = nullptr, *d_Q = nullptr, *d_Vm = nullptr, *d_Va = nullptr;
    hpf::cplx *d_U = nullptr, *d_E = nullptr;
    double* d_f = nullptr;            // [S][N]  mismatch, overwritten by the Newton step during a solve
    hpf::cplx* d_I0 = nullptr;            // [S][n]  network current of the power rows, kept by the harmonic mismatch kernel
    unsigned long long* d_errbits = nullptr;   // [S]   ||f||_inf as the bit pattern of the double (hpf_mismatch: k_err_reduce)
    unsigned long long* d_errpart = nullptr;   // [S][errpart_stride] partial maxima of |f|, one per wavefront of the mismatch launch (k_mismatch)
    int errpart_stride = 0;
    double* d_err = nullptr;          // [S]
    int* d_niter = nullptr;           // [S]
    int* d_active = nullptr;          // [S]
    int* d_nactive = nullptr;         // [1]
    int* d_pivflag = nullptr;         // [S] bit0: a static 4x4 pivot block exceeded piv_limit (k_factor_q), bit1: repeated with partial pivoting,
                                      //     bit2: exactly zero pivot met by the pivoted wave Gauss-Jordan (k_factor_w)
                                      //     bit3: a Newton step missed the residual check (k_step_eta) in the current pass, bit4: ... in the first pass of a repeated scenario
    int resid_check = 0;              // option "step_residual_check": k_step_residual + k_step_eta between the linear solve and the update
    int rect_update = 0;              // option "rectangular_update": launch_update<false> applies the harmonic steps through U (k_update_rect); hpf_stat.flags bit 9
    double resid_limit = 1e-10;       // option "step_residual_limit_log10": eta above it (or not finite) flags the scenario
    unsigned long long* d_respart = nullptr;   // [S][4][errpart_stride] partial maxima of |r|, row sums of |J|, |dx|, |f| (one per wavefront of k_step_residual)
    double* d_eta = nullptr;          // [2][S_alloc] eta of the last step | largest eta of the solve (-1: no step yet)
    int* d_mask = nullptr;            // [S] scenarios of a repeat pass
    double *d_Vm0 = nullptr, *d_Va0 = nullptr;   // [S][Hn*n] state at the entry of hpf_solve (repeat with partial pivoting starts from it)
    double *d_Vmp = nullptr, *d_Vap = nullptr;   // [S][Hn*n] option "keep_previous_state": the state each scenario's LAST Newton step started from
    double *d_swapVm = nullptr, *d_swapVa = nullptr;   // [S][Hn*n] hpf_jacobian(_csr)_last: the current state while the kept one stands in its place
    int queue_chunk = 4;              // option "queue_chunk": iterations between two harvest / refill rounds of hpf_solve_queue
    // distortion accumulator `dist` (hpf_distortion_*, hpf_distortion.hpp).  Entries bus-major like the state: t = i*Hn + q for x of (bus i,
    // harmonic position q), t = n*Hn + i for the THD of bus i; f [3][n*Hn + n], arg [n*Hn + n], over [n*Hn + n] | [n][bins + 1] THD histogram
    bool solve_done = false;          // d_stats / the state belong to a finished hpf_solve of the current batch (hpf_distortion_add)
    bool stats_valid = false;         // d_stats were written by an hpf_solve of the current batch (hpf_get_stats; a new batch -- set_loads, set_state, start_apply, the queue -- ends it)
    int dist_bins = 0;
    int dist_id_base = 0;             // option "distortion_id_base": hpf_solve_queue adds scenario g of a call under id base + g
    double dist_thd_limit = 0.0, dist_hist_max = 0.0, dist_inv_w = 0.0;
    // branch table (hpf_branch.hpp; built by the first call that needs it, absent otherwise): branch e = stored pair (i, j), i < j, numbered in
    // CSR order of its upper-triangle entry
    bool br_built = false;
    int nb = 0;
    std::vector<int> br_from, br_to, br_ypos;   // [nb] host copies (hpf_get_branches); ypos = position of (i, j) in col
    int *d_br_from = nullptr, *d_br_to = nullptr;
    hpf::cplx* d_br_y = nullptr;      // [nb][Hn] series admittances y = -Y, branch-major
    double* d_br_part = nullptr;      // [S_max][tiles][Hn] per-tile sums of loss[q][e] (k_branch_flows -> k_branch_loss_h)
    // branch statistics accumulator `bstat` (hpf_branch_stats_*): f [9][nb] irms, loss, harmonic loss; arg [3][nb]; over [nb] irms above the rating
    // waveform statistics accumulator `wstat` (hpf_waveform_stats_*, hpf_waveform.hpp): f [6][n] peak, crest; arg, over [2][n]
    int ws_T = 0;                     // samples per fundamental period
    double ws_crest_limit = 0.0;
    double *d_ws_ct = nullptr, *d_ws_st = nullptr;   // [T] twiddle table (wave_table)
    int* d_ws_orders = nullptr;       // [Hn] harmonic orders
    double *d_ws_peak = nullptr, *d_ws_crest = nullptr;   // [S_max][n] scratch: k_wave_peaks -> k_wave_add
    // start state (hpf_start_*; allocated while set only): one scenario's Vm, Va, U, E [n*Hn], bus-major like the state
    bool start_set = false;
    bool from_start = false;          // the current batch came from hpf_start_apply (until the next hpf_set_state): hpf_stat.flags bit 8
    double *d_sVm = nullptr, *d_sVa = nullptr;
    hpf::cplx *d_sU = nullptr, *d_sE = nullptr;
    // per-scenario Norton source currents (hpf_set_sources / hpf_queue_sources, hpf_sources.hpp; nothing allocated until the first of them)
    bool src_set = false;             // the current batch has sources: the mismatch and the step-residual kernels launch their source variants, hpf_stat.flags bit 10
    hpf::cplx* d_src = nullptr;       // [S_max][n - m][Hn] I_src, indexed by scenario id like d_P (virtual slots of a meshed handle never form a mismatch: none)
    int qsrc_n = 0, qsrc_form = 0;    // registration of hpf_queue_sources: scenarios (0: none), input form
    void* d_qsrc = nullptr;           // the whole sweep's data in HBM: form 0 [n_total][n - m][Hn] complex, form 1 [n_total][n - m][2] doubles
    int* d_qorders = nullptr;         // [Hn] harmonic orders (form 1)
    int keep_prev = 0;
    bool prev_valid = false;          // d_Vmp / d_Vap belong to the last hpf_solve (set_state / set_loads invalidate them)
    double* d_hist = nullptr;         // [S][hist_cap]
    int hist_cap = 0;
    hpf_stat* d_stats = nullptr;      // [S]
    // dense solver
    double* d_J = nullptr;            // [S_alloc][Nmax*Nmax]
    size_t J_elems_per_scen = 0;
    int J_scen_alloc = 0;
    int* d_ipiv = nullptr;
    int* d_info = nullptr;
    bool info64 = false;              // the last dense factorisation went through rocSOLVER's 64-bit entry points (int64 pivots / info)
    // CSR export of the Jacobian (hpf_jacobian_csr): indptr [N+1] (built once per handle), column indices / values of one scenario
    int* d_jptr = nullptr;
    int* d_jcol = nullptr;
    double* d_jval = nullptr;
    long long jnnz = 0;
    // block-tree solver
    hpf::Tree tree;                   // elimination tree as the network gives it (single-wave / generic kernels, pf)
    hpf::Tree ctree;                  // the same with pass-through buses contracted (multi-wave kernels, gj_mode 1)
    bool has_ctree = false;
    long long n_back_tails = 0;       // back sweeps whose bordered buses and constant-inverse leaves went through k_back_tail (hpf_tree_census[16])
    int last_batch_tile = 0;          // scenarios per batched workgroup of the last factor launch with bordered buses (16 or 8; 0: none yet; CENSUS_BATCH_TILE)
    int last_leaf_tile = 0;           // ... with lazy leaves (CENSUS_LEAF_BATCH_TILE); both written by note_batch_tile at the dispatch sites that launch
    long long n_back_walks = 0;       // back sweeps (scenario group x Newton step) whose Gauss-Jordan buses went through k_back_walk (hpf_tree_census[15])
    int auto_repivot = 1;             // hpf_solve repeats scenarios flagged by the static-pivot monitor with partial pivoting
    int* h_act[2] = {nullptr, nullptr};          // pinned copies of the slot counter d_nactive, and of the queue's `next` (poll_post / poll_wait: the host looks at chunk c - 1 while chunk c runs)
    hipEvent_t poll_ev[2] = {nullptr, nullptr};
    double *trace_Vm = nullptr, *trace_Va = nullptr;   // hpf_set_trace: caller's [S][trace_cap][Hn*n] arrays (per-iteration states)
    int trace_cap = 0;
    // hpf_solve with a trace on a handle that may repeat: the first pass records into trace_stage (the layout of the caller's arrays: Vm, then
    // Va), the repeat pass writes the rows of the scenarios in trace_only alone; trace_last: the last row the pass just finished recorded
    std::vector<double> trace_stage;
    bool trace_staged = false;
    std::vector<int> trace_only;
    int trace_last = 0;
    double* d_Z = nullptr;            // [S][n][b*b]
    double* d_w = nullptr;            // [S][n][b]
    double* d_x = nullptr;            // [S][n][b]  Newton step, bus-major
    long long* d_dbg = nullptr;       // [S][n][8] diagnostic phase stamps of the factor kernel (HPF_DEBUG_ABLATE & 16)
    double* d_C = nullptr;            // [S][n][(B+1)*B] Schur complements pushed by dense children (MFMA mode)
    double* d_H = nullptr;            // [S][n][Hn][4] A(k,parent) blocks of the dense buses, kept for the back sweep
    double* d_chG = nullptr;          // [S][n][Hn][4] contracted tree: A'(top parent, ch) of a chain's bottom dense bus ch
    double* d_chH = nullptr;          // [S][n][Hn][4]                  A'(ch, top parent)
    double* d_chD = nullptr;          // [S][n][Hn][4] harmonic-diagonal addend to the diagonal block of ch
    double* d_chy = nullptr;          // [S][n][Hn][2] addend to the right-hand side of ch
    double* d_fb = nullptr;           // [S][n][Bst] bus-major image of the harmonic mismatch (zeros where there is no equation)
    double* d_lfK = nullptr;          // [S][n][12]    constant-inverse leaves: (c0 + D)^-1 (back sweep, lazy rebuild), G0 S_c^-1, H0 S_parent^-1 (lazy rebuild)
    double* d_lfS = nullptr;          // [S][n][Hn][4] constant-inverse leaves: S_q^-1 (polar <- rectangular), row-major
    double* d_chZ = nullptr;          // [S][n][Hn][4] D_k^-1 A'(k, ch) of the chain buses k (back substitution)
    double* d_linA = nullptr;         // [S][n][Hn][4] inverse 2x2 blocks of the all-linear-subtree buses
    double* d_F = nullptr;            // [S][n_comp][3][tile image] compress steps: A(c,v) D_v^-1 A(v,c) | Gd = A'(p,c) (MFMA A-operand order) | Hd = A'(c,p)
    double* d_H2 = nullptr;           // [S][n_comp][Hn][4] A(v,c) of the compressed buses (back sweep)

    hipStream_t own_stream = nullptr, stream = nullptr;
    int n_groups = 4;                 // (initially sw.n_groups) "scenario_groups"
    hipStream_t gstream[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // groups 1..7 (group 0: the handle's stream, group_stream)
    hipEvent_t fork_ev = nullptr, join_ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    rocblas_handle blas = nullptr;
    double setup_ms[4] = {0, 0, 0, 0}; // hpf_create: total | tree planning on the host | tree uploads | per-scenario allocation
    int timing = 0;                   // hpf_timing_enable: 1 HIP-event spans + device stamps, 2 device stamps only (no event packets between kernels)
    std::vector<hpf::TimedSpan> spans;
    double t_ms[hpf::T_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t t_n[hpf::T_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};
    static constexpr int TS_CAP = 16384;         // launches of the general factor kernel a timing leg can stamp
    unsigned long long* d_tstamp = nullptr;      // [TS_CAP][2] first workgroup start / last workgroup end (wall_clock64) per launch
    int ts_next = 0;

    // Owners of every device block above (hpf_devmem.hpp; declared last: they go first, and null the pointers they hold).  What lives as long as
    // the handle is in `mem`; buffers that come and go share one owner per group, allocated all-or-nothing and released by its clear().
    hpf::DevMem mem{&last_detail};        // model, per-scenario state, both trees, tree scratch, mesh / selected inversion / border, stamps, CSR export, swap, d_hist
    hpf::DevMem br_mem{&last_detail};     // d_br_*
    hpf::DevMem start_mem{&last_detail};  // d_sVm, d_sVa, d_sU, d_sE
    hpf::DevMem src_mem{&last_detail};    // d_src
    hpf::DevMem qsrc_mem{&last_detail};   // d_qsrc, d_qorders
    hpf::DevMem repeat_mem{&last_detail}; // d_Vm0, d_Va0, d_mask
    hpf::DevMem prev_mem{&last_detail};   // d_Vmp, d_Vap
    hpf::DevMem resid_mem{&last_detail};  // d_respart, d_eta
    hpf::DevMem dense_mem{&last_detail};  // d_J, d_ipiv, d_info
    hpf::Accum dist{&last_detail}, bstat{&last_detail}, wstat{&last_detail};   // the sweep accumulators (wstat.mem: d_ws_* too)
};

namespace hpf {

// status of the kernel launches since the last check: HPF_OK, or HPF_E_HIP with the HIP error in last_detail
inline int launch_status(hpf_handle* h) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return HPF_OK;
    h->last_detail = (int)e;
    return HPF_E_HIP;
}

// Stream of scenario group g: group 0 runs on the handle's stream itself, so a step of G groups keeps G hardware queues busy, not G + 1 (the
// runtime maps streams onto four queues; a fifth busy stream shares one and serialises two groups: 1.25 instead of 0.90 ms per step at G = 4)
inline hipStream_t group_stream(const hpf_handle* h, int g) { return g == 0 ? h->stream : h->gstream[g]; }

// Launch context: the stream and the scenario slice [s0, s0 + S) a launch helper targets, and the slot list of the slice (nullptr: every
// scenario of it).  A value handed down the call chain -- scenario groups run as independent pipelines on their own streams, so that the
// latency-bound upper tree levels of one group overlap the others, and a nested sweep (the bordered step) builds its own.
struct LaunchCtx { hipStream_t stream; int s0, S; const int* active; };
// the whole batch on the handle's stream
inline LaunchCtx batch_ctx(const hpf_handle* h, const int* active = nullptr) { return {h->stream, 0, h->S, active}; }

// which part of tree_newton_step runs (BACK_ONLY: the second pass of the factor-once bordered step)
enum TreePass { FACTOR_AND_BACK, BACK_ONLY };

// words of hpf_tree_census behind the tree's own eight (Tree::census), in the ABI's order (device.py: tree_census names them alike)
enum CensusWord {
    CENSUS_TIES = 8, CENSUS_FUSED_LEVELS, CENSUS_COMPRESS_STEPS, CENSUS_BORDER_REPIVOTS, CENSUS_BORDER_UNKNOWNS, CENSUS_ROOT_PATH_BUSES,
    CENSUS_BORDERED_FORM, CENSUS_BACK_WALKS, CENSUS_BACK_TAILS, CENSUS_BATCH_TILE, CENSUS_LEAF_BATCH_TILE, CENSUS_WORDS
};

struct ScopedTimer {
    hpf_handle* h;
    int which;
    hipStream_t stream;               // the stream the span is recorded on: the launch context's
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ScopedTimer(hpf_handle* h_, int w, hipStream_t st) : h(h_), which(w), stream(st) {
        if (h->timing == 1) {
            hipEventCreate(&e0);
            hipEventCreate(&e1);
            hipEventRecord(e0, stream);
        }
    }
    ~ScopedTimer() {
        if (h->timing == 1) {
            hipEventRecord(e1, stream);
            h->spans.push_back({which, e0, e1});
        }
    }
};

// block-tree solver (hpf_block.hip)
int tree_find_ties(hpf_handle* h, const hpf_desc* d);    // spanning tree + loop-closing lines of the pattern (before any allocation)
int tree_build(hpf_handle* h, const hpf_desc* d);
int tree_plan_dump(const hpf_desc* d, const char* path);  // host-only planning run (hpf_tree_plan), no device touched
hpf::Tree& active_tree(hpf_handle* h);
bool tree_levels_fused(hpf_handle* h);                   // every elimination level of the current mode is one k_level launch
int tree_alloc_scenarios(hpf_handle* h);
int tree_fund_step(hpf_handle* h, const LaunchCtx& ctx);   // fundamental pf Newton step on the tree (2x2 blocks)
int tree_newton_step(hpf_handle* h, const LaunchCtx& ctx, TreePass pass);   // assembles, eliminates, back-substitutes -> d_f holds the step
int tree_newton_step_bordered(hpf_handle* h, const LaunchCtx& ctx);   // the same for a network with loop-closing lines (h->n_ties > 0)
int ensure_blas(hpf_handle* h);                                   // rocBLAS handle on first use (dense LU, border system)
int border_slots(const hpf_handle* h);                            // virtual scenario slots of the bordered step (behind the S_max real ones)
int tree_sel_build(hpf_handle* h, const hpf_desc* d);             // factor-once bordered step: P, forward pairs, block-product jobs, buffers (after tree_build)

}  // namespace hpf
