/*
 * libhpf — MI355X (gfx950) harmonic power-flow Newton-Raphson hot path, C ABI.
 *
 * This is the drop-in boundary for ONE path of pweigmann/harmonic-power-flow: the NR loop of
 * `hpf()` in `Harmonic Power Flow/hcne_generalized.py` (HG).  The reference has no FFI of its own (its hot path
 * sits behind plain Python functions, HG:360-560); each entry point below names the reference function it
 * replaces.  The Python host (`harmonic-power-flow_amd/`) binds these symbols with `ctypes` and re-exports the
 * reference's own call shapes (`hpf`, `pf`, `harmonic_mismatch`, `build_harmonic_jacobian`, ...).
 *
 * Conventions
 *   - return 0 on success; < 0 invalid argument / wrong state; > 0 device-side failure (HIP, rocSOLVER, singular
 *     pivot): see hpf_strerror().  Nothing throws across the ABI.
 *   - all host buffers are caller-owned and copied in/out; `*_dev` entry points take device pointers instead.
 *   - the handle owns all device memory, one HIP stream and the rocBLAS handle; one handle per (process, device).
 *     A handle is not thread-safe; distinct handles are independent.
 *   - complex128 arrays are interleaved (re, im) doubles, NumPy layout.
 *   - all arithmetic is FP64.  Stacked index k = q*n + i (harmonic position q, bus i), HG:139-143.
 *   - scenarios: S independent load cases (P, Q per bus) share topology, admittances and Norton data; every
 *     per-scenario array is [S][...] with the scenario index slowest.
 */
#ifndef HPF_H
#define HPF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hpf_handle hpf_handle;

enum {
    HPF_SOLVER_DENSE = 0,      /* dense real FP64 Jacobian, rocSOLVER getrf/getrs (any topology).  N*N < 2^31 (N <= 46 340): the batched
                                  32-bit entry points; larger systems (8 N^2 bytes per scenario: 21.6 GB at N = 51 998) go through
                                  rocSOLVER's 64-bit entry points one scenario after the other; HPF_E_NOMEM when they do not fit */
    HPF_SOLVER_BLOCK_TREE = 1  /* bus-major 2Hn x 2Hn block elimination along the feeder tree.  Radial networks directly; meshed
                                  networks as BFS spanning tree + k loop-closing lines, solved as a bordered system on top of the
                                  same tree factorisation (m = 2Hn x number of distinct endpoint buses of the loop-closing lines;
                                  two sweeps of the tree per scenario and Newton step + a selected inversion over the endpoints' root
                                  paths; uncoupled models and HPF_MESH_SEL=0: m + 2 right-hand sides as virtual scenarios in chunks
                                  of up to 1 024; m x m border system on rocSOLVER); m <= 16 384 and 2Hn <= 100, else HPF_E_TOPOLOGY */
};

enum {
    HPF_OK = 0,
    HPF_E_ARG = -1,        /* null pointer / out-of-range argument */
    HPF_E_STATE = -2,      /* call order violated (e.g. solve before loads were set) */
    HPF_E_TOPOLOGY = -3,   /* BLOCK_TREE: network not connected from bus 0 / pattern not symmetric / border of the loop-closing lines
                              beyond the stated bound */
    HPF_E_NOMEM = -4,
    HPF_E_HIP = 1,         /* HIP runtime error (hpf_last_error_detail has the hipError_t) */
    HPF_E_ROCSOLVER = 2,   /* rocBLAS / rocSOLVER status != success */
    HPF_E_SINGULAR = 3     /* a factorisation met an exactly zero pivot */
};

/* Model description (host pointers, copied by hpf_create).  Produced by the Python ingest from the reference's CSV
 * formats: bus/line CSVs -> (n, m, c) HG:113-128; per-harmonic admittances HG:132-171 stored as one CSR pattern
 * shared by all harmonics; Norton equivalents HG:278-310 per device type. */
typedef struct hpf_desc {
    int32_t n;                 /* buses                                                            HG:126 */
    int32_t m;                 /* 0-based index of first nonlinear bus (n if none)                 HG:122-125 */
    int32_t c;                 /* number of PV buses + 1                                           HG:127 */
    int32_t Hn;                /* harmonics incl. fundamental (K+1)                                HG:584 */
    int32_t nnz;               /* stored entries of the shared admittance pattern (full diagonal present) */
    int32_t n_dev;             /* nonlinear device types                                           HG:285 */
    int32_t coupled;           /* 1: Y_N is Hn x Hn per device; 0: Y_N is a length-Hn vector       HG:301-308 */
    int32_t solver;            /* HPF_SOLVER_*                                                             */
    int32_t device;            /* HIP device ordinal                                                       */
    int32_t max_scenarios;     /* capacity S_max >= 1                                                      */
    const int32_t* rowptr;     /* [n+1]                                                                    */
    const int32_t* col;        /* [nnz], ascending inside a row                                            */
    const double*  Yval;       /* [Hn][nnz] complex128                                                     */
    const int32_t* dev_of_bus; /* [n]: device type of a nonlinear bus, -1 for linear buses                 */
    const double*  Y_N;        /* coupled: [n_dev][Hn][Hn] complex128 (row = harmonic of injected current,
                                  col = harmonic of voltage, HG:304,432); uncoupled: [n_dev][Hn]           */
    const double*  I_N;        /* [n_dev][Hn] complex128                                                   */
} hpf_desc;

/* Per-scenario result record, also the payload of the multi-GPU statistics gather (24 bytes). */
typedef struct hpf_stat {
    int32_t n_iter;            /* harmonic NR iterations performed                       HG:542 */
    int32_t flags;             /* bit0 converged (err <= thresh), bit1 hit max_iter, bit2 non-finite mismatch,
                                  bit3 BLOCK_TREE: a static 4x4 pivot block amplified beyond the limit during the solve,
                                  bit4 the scenario was repeated with partial pivoting (its result is the repeat's),
                                  bit5 the pivoted elimination met an exactly zero pivot (hpf_solve returns HPF_E_SINGULAR),
                                  bit6 option "step_residual_check": a Newton step of the first pass missed the residual limit,
                                  bit7 ... a step of the pass whose result is returned did (= bit6 unless bit4 is set),
                                  bit8 the scenario was started from the handle's start state (hpf_start_*), not from the reference's start + pf,
                                  bit9 the scenario's harmonic steps were applied in rectangular form (option "rectangular_update"),
                                  bit10 the scenario was solved with per-scenario source currents (hpf_set_sources / hpf_queue_sources) */
    double  err;               /* final ||f||_inf                                        HG:389 */
    double  thd_max;           /* max over buses of THD_F                                HG:566-568 */
} hpf_stat;

int  hpf_create(hpf_handle** out, const hpf_desc* d);
/* hpf_create with build switches for THIS handle: `options` = "NAME=value NAME=value ..." (separators: space, comma, semicolon; NULL or "" = none)
 * with the HPF_* names listed at hpf_set_option below ("Switches read by hpf_create").  The process environment is consulted for the same names
 * ONLY when the process opts in with HPF_ENV_SWITCHES=1 (A/B tooling, the test-suite): without it nothing a handle computes depends on
 * environment variables.  hpf_create(out, d) = hpf_create_opts(out, d, NULL). */
int  hpf_create_opts(hpf_handle** out, const hpf_desc* d, const char* options);
int  hpf_destroy(hpf_handle* h);
const char* hpf_strerror(int code);
int  hpf_last_error_detail(const hpf_handle* h);      /* hipError_t / rocblas_status / pivot index of the last >0 code */
int  hpf_version(void);

/* Sizes: N = 2*n*Hn - 1 - c unknowns of the harmonic NR (HG:388,397); Nf = 2*n - 1 - c of the fundamental NR. */
int  hpf_num_unknowns(const hpf_handle* h);
int  hpf_num_unknowns_fund(const hpf_handle* h);
/* Scenario counts, so that a host binding sizes the per-batch output arrays below from the LIBRARY and not from a mirror of its own: S = the
 * current batch (set by hpf_set_loads / hpf_set_state; 0 when the handle holds no batch, e.g. right after hpf_create or hpf_solve_queue) and the
 * capacity S_max of hpf_create.  Every per-batch output ([S][...] below) is written for exactly hpf_num_scenarios() scenarios; per-batch calls on a
 * handle without a batch return HPF_E_STATE. */
int  hpf_num_scenarios(const hpf_handle* h);
int  hpf_max_scenarios(const hpf_handle* h);
/* BLOCK_TREE: number of elimination levels of the dense tree (= factor-kernel launches per Newton step and scenario group;
 * pass-through buses are contracted first in the default mode) / of back-substitution levels; 0 for DENSE. */
int  hpf_tree_levels(const hpf_handle* h);
int  hpf_tree_depths(const hpf_handle* h);

/* Loads P,Q [S][n] in p.u. (buses.P / buses.Q of HG:197,372).  Sets the active scenario count S.
 * Call order of a batch (tests/handle_contract.py is this paragraph as a table).  hpf_set_loads opens a batch: n_scen outside 1 .. S_max is
 * HPF_E_ARG and leaves the handle as it was.  A state of the SAME n_scen is kept -- new loads for the state the handle holds, as a sweep's re-solve
 * uses it, and hpf_stat.flags bit 8 of a state that came from hpf_start_apply stays with it; a state of another n_scen is dropped (hpf_get_state
 * and every call that needs a state then return HPF_E_STATE until the next hpf_set_state / hpf_start_apply).  Sources, the mismatch, the kept
 * previous state and the records of the last hpf_solve do not survive hpf_set_loads.  hpf_set_state / hpf_start_apply with loads set take the
 * loads' n_scen only (HPF_E_ARG otherwise: change the batch size with hpf_set_loads first); they keep loads and sources and end the mismatch, the
 * previous state and the records.  A call refused by a check on the host (code < 0, before any device work) changes nothing: not the batch, not
 * hpf_num_scenarios, not an option -- with one exception, hpf_solve_queue refusing a registration of hpf_queue_sources, which drops the
 * registration.  (hpf_start_capture answering HPF_E_STATE for a scenario with a non-finite or zero entry is no such refusal: its kernel found
 * the entry while overwriting the start buffers, and the handle is left without a start state, as stated there.)  Where a call could be refused for its
 * arguments and for the handle's state, the argument ranges that do not depend on the state (n_scen against S_max, an unknown form, a NULL
 * pointer, scen < 0) come first, then the state, then the arguments that are measured against the batch (n_scen against S, scen >= S). */
int  hpf_set_loads(hpf_handle* h, int n_scen, const double* P, const double* Q);
/* Voltages Vm,Va [S][Hn*n] (the V DataFrame of HG:174-184, signed magnitudes allowed).  NULL,NULL -> the reference's
 * initial values (1 p.u. at h=1, 0.1 p.u. above, angle 0; init_voltages HG:174-184) for all S scenarios. */
int  hpf_set_state(hpf_handle* h, int n_scen, const double* Vm, const double* Va);
int  hpf_get_state(hpf_handle* h, double* Vm, double* Va);      /* raw: signed, un-wrapped; host applies HG:545-549 */

/* harmonic_mismatch (HG:360-390) incl. current_balance / current_injections (HG:313-357) for all S scenarios.
 * f [S][N] (may be NULL), err [S] (may be NULL). */
int  hpf_mismatch(hpf_handle* h, double* f, double* err);
/* build_harmonic_jacobian (HG:401-473) of scenario `scen`, written as a dense column-major N x N matrix
 * (parity / debugging; the solver consumes the device copy directly). */
int  hpf_jacobian(hpf_handle* h, int scen, double* J_colmajor);
/* The Jacobian the reference's hpf() returns (HG:537,560): the one of the LAST iteration of the last hpf_solve, i.e. built at the
 * state scenario `scen`'s last Newton step started from (needs option "keep_previous_state" = 1 before hpf_solve; the current state
 * is left untouched).  HPF_E_STATE, checked on the host: option off, no batch, no hpf_solve with the option on since the batch's loads and state
 * were set (hpf_mismatch, hpf_iterate and hpf_fund_pf do not end it: the kept state stays the last hpf_solve's), or a scenario that took no step
 * in that solve.  The option may be switched off and on again in between: the kept state survives. */
int  hpf_jacobian_last(hpf_handle* h, int scen, double* J_colmajor);
/* build_harmonic_jacobian (HG:401-473) in the form the reference returns it from build_harmonic_jacobian and from hpf() (HG:469-472,
 * HG:560): the stacked real matrix [[dP/dth dP/dV] [Re dI/dth Re dI/dV] [dQ/dth dQ/dV] [Im dI/dth Im dI/dV]] as CSR -- indptr [N+1],
 * indices [nnz] (ascending inside a row), data [nnz] = the three arrays of scipy.sparse.csr_matrix.  Assembled on the device entry by
 * entry straight into the CSR arrays (no dense N x N anywhere: 14.7 MB at the 1 000-bus x 26-harmonic feeder where the dense copy is
 * 21.6 GB).  The pattern is a property of the model (admittance pattern + Norton coupling: what the reference's block_diag / lil
 * construction stores; entries that only vanish by cancellation at a particular state stay stored); hpf_jacobian_nnz sizes the arrays.
 * indptr / indices may be NULL on repeated calls (values only).  HPF_E_ARG if nnz would not fit 32-bit indices.
 * hpf_jacobian_csr_last: at the state the scenario's last Newton step started from, like hpf_jacobian_last. */
int  hpf_jacobian_nnz(hpf_handle* h, int64_t* nnz);
int  hpf_jacobian_csr(hpf_handle* h, int scen, int32_t* indptr, int32_t* indices, double* data);
int  hpf_jacobian_csr_last(hpf_handle* h, int scen, int32_t* indptr, int32_t* indices, double* data);
/* fund_mismatch + build_jacobian of the fundamental power flow (HG:195-223) for scenario `scen`: f [Nf], J [Nf*Nf]. */
int  hpf_fund_mismatch(hpf_handle* h, double* f, double* err);
int  hpf_fund_jacobian(hpf_handle* h, int scen, double* J_colmajor);

/* pf (HG:244-275): fundamental NR from the current state for all S scenarios; leaves the harmonic rows untouched.
 * n_iter [S], err [S] may be NULL.  err_hist [S][max_iter] (HG:264, may be NULL). */
int  hpf_fund_pf(hpf_handle* h, double thresh, int max_iter, int* n_iter, double* err, double* err_hist);

/* The NR loop of hpf (HG:530-542) from the current state: initial mismatch, then while err > thresh and
 * n_iter < max_iter: Jacobian -> solve -> update -> mismatch.  Scenarios that satisfy the stop rule freeze.
 * n_iter [S], err [S], err_hist [S][max_iter+1] (initial + one per iteration; unused tail = NaN) may be NULL.
 * BLOCK_TREE (static pivot order on the matrix cores): every 4x4 pivot block is watched; a scenario in which one amplifies
 * rounding errors by more than the limit (option "pivot_growth_limit_log10", default 10), or whose mismatch turns non-finite,
 * is repeated from the state the call was entered with, with partial pivoting over the whole bus block (flags bit3 / bit4).
 * Returns HPF_E_SINGULAR (detail = scenario; outputs are still written) if a pivoted elimination met an exactly zero pivot --
 * DENSE: rocSOLVER info > 0, BLOCK_TREE: the pivoted wave Gauss-Jordan. */
int  hpf_solve(hpf_handle* h, double thresh, int max_iter, int* n_iter, double* err, double* err_hist);

/* A sweep of n_total scenarios through the handle's S_max slots -- the reference's counterpart is one hpf() call per load case (HG:511:
 * other buses.P / buses.Q, HG:197,372).  P, Q [n_total][n] in p.u.  Every scenario: the reference's start (HG:174-184), pf (HG:244-275) with
 * (thresh_f, max_iter_f), the harmonic NR of hpf_solve with (thresh, max_iter).  Radial BLOCK_TREE handles keep all loads and pf seeds in HBM
 * and, between chunks of Newton iterations (option "queue_chunk", default 4), harvest the scenarios that met the stop rule and put the next
 * pending scenarios into the freed slots, so the handle stays full until the queue drains; every scenario's result is bit-identical to its
 * solve alone (the arithmetic of a scenario does not depend on its slot).  Other handles (DENSE, meshed networks, pivoted mode) run waves of
 * S_max scenarios.  Outputs (host, may be NULL; Vm and Va together): stats [n_total], raw voltages Vm, Va [n_total][Hn*n] (stacked order,
 * signed / un-wrapped like hpf_get_state).  In the queued mode a scenario flagged by the static-pivot monitor (flags bit 3) or whose mismatch
 * turned non-finite (flags bit 2), or whose step missed the residual check (flags bit 6), is reported, not repeated: solve it again with hpf_solve (which repeats exactly those with partial pivoting).  Afterwards the handle holds no batch: set loads and state before per-batch calls.
 * With a start state set (hpf_start_set / hpf_start_capture below) every scenario begins at that state instead: no pf phase -- thresh_f and
 * max_iter_f are IGNORED -- and every record carries flags bit 8. */
int  hpf_solve_queue(hpf_handle* h, int n_total, const double* P, const double* Q, double thresh_f, int max_iter_f, double thresh,
                     int max_iter, hpf_stat* stats, double* Vm, double* Va);

/* Per-iteration state dump for trajectory diffing against the oracle / the reference (the reference's analogue is the JSON log of
 * every iterate, hcne_based_on_fuchs.py:186,370-372): while set, hpf_solve writes the voltages after iteration k (k = 0: the
 * state it was entered with) of every scenario to Vm_traj / Va_traj [S][cap][Hn*n] (caller-owned host arrays, stacked order
 * q*n + i; frozen scenarios repeat their last state; iterations >= cap are not recorded).  The solve then synchronises with the
 * host after every iteration.  Rows 0 .. L are written, L = the largest n_iter among the results the call returns; rows beyond L are left
 * as the caller filled them.  Where hpf_solve repeats scenarios with partial pivoting (flags bit 4), the rows of a repeated scenario are the
 * repeat's (row 0: the entering state) and the rows of every other scenario those of the first pass: no row holds a state of a pass the
 * scenario's result does not come from.  (Such a handle keeps the first pass in a host copy of the size of the two arrays until it knows which
 * scenarios are repeated.)  NULL, NULL, 0 switches it off. */
int  hpf_set_trace(hpf_handle* h, double* Vm_traj, double* Va_traj, int cap);

/* One unconditional NR iteration (Jacobian -> solve -> update -> mismatch) for all S scenarios, repeated `iters`
 * times, no host synchronisation inside (throughput measurement; update_harmonic_state_vec HG:476-479 +
 * update_harmonic_voltages HG:482-485).  Requires a valid mismatch: hpf_mismatch after the last call that set loads, sources or state and after
 * the last hpf_solve / hpf_fund_pf (scenarios those froze hold stale mismatch rows); HPF_E_STATE otherwise.  hpf_iterate itself leaves the
 * mismatch valid.  It ends "hpf_solve was the last call that touched the batch" for the accumulators' add; the records of hpf_get_stats stay
 * those of the last hpf_solve. */
int  hpf_iterate(hpf_handle* h, int iters);

/* update_harmonic_state_vec (HG:476-479) as a standalone, stateless call like the reference's: dx = J^-1 f for a dense
 * column-major N x N Jacobian supplied by the caller (rocSOLVER LU, partial pivoting); the caller forms x - dx.  N * N >= 2^31 goes through
 * rocSOLVER's 64-bit entry points; HPF_E_NOMEM (before anything is allocated) when 8 N^2 bytes do not fit the device's free memory. */
int  hpf_dense_solve(int device, int N, const double* J_colmajor, const double* f, double* dx);
/* The same call for the Jacobian in the form the reference passes it (HG:478: the scipy CSR matrix build_harmonic_jacobian returns, HG:469-472),
 * at every size: indptr [N + 1], indices [nnz], data [nnz] of the N x N matrix in the reference's stacked row / column order, N = 2 n Hn - 1 - c
 * (n buses, c = PV buses + 1, Hn harmonics: the numbering is a function of these three alone), f [N] -> dx [N] = J^-1 f.  The entries are
 * scattered on the device into bus-major 2 Hn x 2 Hn blocks and eliminated along the feeder tree (partial pivoting inside a bus block; off-diagonal
 * blocks may be dense); no N x N array exists on host or device (65 MB of blocks at 1 000 buses x 26 harmonics, where the dense matrix is
 * 21.6 GB).  Duplicate (row, column) entries add up like scipy's.  A MESHED bus graph (spanning tree + loop-closing lines) is solved as a bordered
 * system: the tree part is factorised once, a selected inversion over the root paths of the lines' endpoint buses gives the m x m border matrix
 * (m = 2 Hn x number of distinct endpoint buses <= 16 384; rocSOLVER LU), one more right-hand-side sweep the solution (1 000 buses x 26 harmonics
 * + 20 lines: 27 ms, 1e-12 of the step from SuperLU).  HPF_E_TOPOLOGY when the bus graph is not connected from bus 0, the block pattern is not
 * symmetric (a block (i, j) without (j, i)) or the border exceeds that bound -- use hpf_dense_solve where it fits --, HPF_E_ARG for 2 Hn > 128 or an
 * inconsistent CSR, HPF_E_SINGULAR when a bus block or the border system has no pivot.  Stateless like the reference's function: no handle.
 * Pivoting stays inside a bus block and only an EXACTLY zero pivot is reported: a near-singular bus block of a nonsingular J returns an
 * inaccurate dx with HPF_OK, and an exactly singular one HPF_E_SINGULAR where a dense LU would succeed.  A C caller gets no residual check;
 * check |f - J dx| itself and fall back to hpf_dense_solve (the Python update_harmonic_state_vec does both).
 * (env HPF_SPARSE_INFO=1 prints its phase times to stderr.) */
int  hpf_sparse_solve(int device, int n, int c, int Hn, const int32_t* indptr, const int32_t* indices, const double* data, const double* f,
                      double* dx);

/* Per-scenario statistics after hpf_solve; `thd_max` from get_THD (HG:563-572) evaluated on device.  The records are those of the last hpf_solve
 * of the CURRENT batch (an hpf_solve that returned HPF_E_SINGULAR included: its outputs are written): HPF_E_STATE without a batch, and after
 * hpf_set_loads / hpf_set_state / hpf_start_apply until the next hpf_solve -- never the records of an earlier batch.  hpf_mismatch, hpf_iterate,
 * hpf_fund_pf and the source calls leave them as they are. */
int  hpf_get_stats(hpf_handle* h, hpf_stat* stats /* [S] host */);
int  hpf_get_stats_dev(hpf_handle* h, void* stats_dev /* [S] hpf_stat, device memory of the caller (RCCL gather) */);

/* Residual check of the Newton steps (option "step_residual_check"): eta_last [S] the normwise backward error
 * eta = |f - J dx|_inf / (| |J| |_inf |dx|_inf + |f|_inf) of every scenario's last harmonic Newton step, eta_max [S] the largest one since
 * hpf_solve was entered (since hpf_set_state for hpf_iterate; after a pivoted repeat: of the repeat).  NaN for a scenario that took no step.
 * Either array may be NULL.  HPF_E_STATE with the check off or without a state (no batch, or loads alone). */
int  hpf_get_step_residuals(hpf_handle* h, double* eta_last, double* eta_max);

/* Distortion accumulator: per-bus / per-harmonic statistics of a sweep, accumulated on the device (the reference's counterpart is a loop of hpf() calls
 * with get_THD, HG:563-572, and a reduction of all returned voltages on the host).  While the accumulator of a handle is open, every scenario that
 * finishes CONVERGED is folded into small device arrays, from the raw signed magnitudes Vm the handle holds (q = harmonic position, i = bus):
 *   x[0][i] = |Vm[0][i]| (fundamental, p.u.),  x[q][i] = |Vm[q][i]| / |Vm[0][i]| for q >= 1 (individual harmonic distortion),
 *   thd[i] = sqrt(sum_{q>=1} Vm[q][i]^2) / |Vm[0][i]| (the arithmetic of hpf_stat.thd_max: sequential sum over ascending q).
 * One thread owns one entry and walks the scenarios (k_distortion_add, one launch per harvest round of hpf_solve_queue / per hpf_distortion_add; no
 * floating-point atomics): max, arg and the integer counters are bit-identical whatever the slot count, queue chunk, scenario groups or number of
 * GPUs; only the four sum arrays depend on the order in which scenarios finish, by rounding alone.  Closed (the default): nothing is allocated, no
 * kernel is launched, every output of every entry point is unchanged; open: records and voltages are unchanged too (it only reads the state).
 * hpf_distortion_begin: allocate, zero, open; on an open accumulator: reset.  limit [Hn] (NULL: +inf) and thd_limit: the `over` arrays count the
 *   scenarios with x[q][i] > limit[q] / thd[i] > thd_limit (strictly).  The THD histogram has hist_bins (1..256) uniform bins on [0, hist_max) and
 *   an overflow bin: bin = thd >= hist_max ? hist_bins : (int)(thd * inv_w), inv_w = hist_bins / hist_max formed once in double.  HPF_E_ARG for
 *   bins outside 1..256, hist_max not in (0, inf), a NaN limit.
 * hpf_distortion_add: fold the handle's CURRENT BATCH in, scenario s under id first_id + s (first_id >= 0).  HPF_E_STATE without a batch, unless
 *   hpf_solve was the last call that touched the batch, or with the accumulator closed.  A scenario that did not converge (hpf_stat.flags bit 0
 *   clear) or has a non-finite thd counts as skipped.
 * hpf_solve_queue with the accumulator open folds every scenario in by itself, under id base + g (g = its index in the call, base = option
 *   "distortion_id_base", so that a sweep cut into several calls keeps global ids) -- every solver and path (the waves of DENSE / meshed / pivoted
 *   handles after each wave).  A scenario whose record has flags bit 2, 3 or 6 (the ones the queue reports for a re-solve through hpf_solve) is NOT
 *   added but counted as deferred: the caller's re-solve adds it with hpf_distortion_add.
 * hpf_distortion_get: copies out whichever arrays are non-NULL, in the ABI's stacked order; leaves the accumulator open.  HPF_E_STATE when closed.
 *   counts [3] int64: scenarios added, skipped, deferred
 *   x_max [Hn][n] double, x_arg [Hn][n] int32: largest x and the id of the scenario it came from (ties: the smallest id; 0 / -1 before the first add)
 *   x_sum, x_sumsq [Hn][n] double: sum of x, of x^2 over the added scenarios;  x_over [Hn][n] uint32: scenarios with x > limit[q]
 *   thd_max [n] double, thd_arg [n] int32, thd_sum, thd_sumsq [n] double, thd_over [n] uint32: the same five for thd[i] against thd_limit
 *   thd_hist [n][hist_bins + 1] uint32: histogram of thd[i], last bin = overflow
 * hpf_distortion_end: free (HPF_OK when already closed); hpf_destroy frees an open one.  All four: HPF_E_ARG for a NULL handle, before any HIP call. */
int  hpf_distortion_begin(hpf_handle* h, const double* limit, double thd_limit, double hist_max, int hist_bins);
int  hpf_distortion_add(hpf_handle* h, int first_id);
int  hpf_distortion_get(hpf_handle* h, int64_t* counts, double* x_max, int32_t* x_arg, double* x_sum, double* x_sumsq, uint32_t* x_over,
                        double* thd_max, int32_t* thd_arg, double* thd_sum, double* thd_sumsq, uint32_t* thd_over, uint32_t* thd_hist);
int  hpf_distortion_end(hpf_handle* h);

/* Branch flows: harmonic currents, RMS loading and series losses of the lines, on the device.  The reference has no counterpart (its
 * current_balance, HG:326-357, forms bus injections only).
 * A BRANCH is one stored off-diagonal pair (i, j), i < j, of the shared admittance pattern.  Branches are numbered in CSR order of their
 * upper-triangle entry (row-major, columns ascending): a function of the pattern alone, radial lines and loop-closing lines alike.  The reference
 * writes Y[from,to] = -1/(R + j h X) and lets a later parallel line overwrite an earlier one (HG:150-155), so a branch is the line the matrix actually
 * contains; its series admittance at harmonic position q is y[q][e] = -Y[q][pos(i,j)].  Shunt parts (HG:157-168) stay out: only the series element
 * carries the conductor current.  Per scenario, with U the rectangular voltages (p.u.):
 *   I[q][e]    = y[q][e] (U[i][q] - U[j][q])          complex, p.u., positive from the lower-numbered bus to the higher
 *   loss[q][e] = Re(y[q][e]) |U[i][q] - U[j][q]|^2    (= R |I|^2, never negative)
 *   irms[e] = sqrt(sum_q |I[q][e]|^2),  thd_i[e] = sqrt(sum_{q>=1} |I[q][e]|^2) / |I[0][e]|  (inf / NaN where the fundamental current is zero),
 *   loss_e[e] = sum_q loss[q][e],  loss_harm[e] = sum_{q>=1} loss[q][e],  loss_h[q] = sum_e loss[q][e].
 * Every product and sum is rounded on its own; every sum over q runs sequentially over ascending q in one thread (|I[0]| = sqrt(|I[0]|^2)); the sum
 * over e of loss_h runs in tiles of 32 consecutive branches -- ascending e inside a tile from 0.0, then the tile sums in ascending tile order from
 * 0.0 -- an order that depends on the number of branches alone.  No atomics.
 * hpf_num_branches: nb (counted by hpf_create; no device call).  hpf_get_branches: from [nb], to [nb] (bus indices, from < to), ypos [nb] (position
 *   of (from, to) in `col`); any pointer may be NULL.  The first of hpf_get_branches / hpf_branch_flows / hpf_branch_stats_begin builds the handle's
 *   branch table (from, to, ypos and a branch-major copy [nb][Hn] of y) on the device; a handle that never calls them holds none.
 * hpf_branch_flows: evaluates at the handle's CURRENT STATE -- after hpf_solve, or after hpf_set_state alone (the rectangular voltages are refreshed
 *   from the state first); every solver, handles used for assembly only included.  Outputs for the hpf_num_scenarios scenarios of the batch, any
 *   pointer may be NULL: I [S][Hn][nb] complex (interleaved re, im), irms / thd_i / loss / loss_harm [S][nb], loss_h [S][Hn].  HPF_E_STATE without a
 *   batch (no state set, or after hpf_solve_queue); HPF_E_ARG for more than 160 harmonics.
 * Branch statistics of a sweep (the twin of the distortion accumulator above: same state rules, same scenario lists, same rule for who is added --
 *   converged scenarios with a finite THD; a scenario hpf_solve_queue only reports, flags bit 2 / 3 / 6, is deferred to the caller's re-solve --
 *   same ids: hpf_solve_queue numbers scenarios through "distortion_id_base", which serves both accumulators).  One thread owns one branch and
 *   walks the finished scenarios (k_branch_add, launched where k_distortion_add is): max, arg, over and counts do not depend on slot count, queue
 *   chunk, scenario groups or number of GPUs; the sums do by rounding alone.  Closed (the default): nothing is allocated or launched.
 * hpf_branch_stats_begin: allocate, zero, open (on an open one: reset).  rating [nb] in p.u. (NULL: +inf); HPF_E_ARG for a NaN rating.
 * hpf_branch_stats_add: fold the current batch in, scenario s under id first_id + s (first_id >= 0); HPF_E_STATE unless hpf_solve was the last call
 *   that touched the batch, or with the accumulator closed.
 * hpf_branch_stats_get: copies out whichever arrays are non-NULL; leaves the accumulator open.  HPF_E_STATE when closed.
 *   counts [3] int64: scenarios added, skipped, deferred
 *   irms_max [nb] double, irms_arg [nb] int32 (ties: the smallest id; 0 / -1 before the first add), irms_sum, irms_sumsq [nb] double,
 *   irms_over [nb] uint32: scenarios with irms[e] > rating[e] (strictly)
 *   loss_max, loss_arg, loss_sum, loss_sumsq: the same four for loss_e;  lossh_max, lossh_arg, lossh_sum, lossh_sumsq: for loss_harm
 *   (thd_i is not accumulated: where a branch carries no fundamental current its samples are inf, NaN or rounding noise)
 * hpf_branch_stats_end: free (HPF_OK when already closed); hpf_destroy frees an open one and the branch table.
 * All of them: HPF_E_ARG for a NULL handle, before any HIP call. */
int  hpf_num_branches(const hpf_handle* h);
int  hpf_get_branches(hpf_handle* h, int32_t* from, int32_t* to, int32_t* ypos);
int  hpf_branch_flows(hpf_handle* h, double* I, double* irms, double* thd_i, double* loss, double* loss_harm, double* loss_h);
int  hpf_branch_stats_begin(hpf_handle* h, const double* rating);
int  hpf_branch_stats_add(hpf_handle* h, int first_id);
int  hpf_branch_stats_get(hpf_handle* h, int64_t* counts, double* irms_max, int32_t* irms_arg, double* irms_sum, double* irms_sumsq,
                          uint32_t* irms_over, double* loss_max, int32_t* loss_arg, double* loss_sum, double* loss_sumsq, double* lossh_max,
                          int32_t* lossh_arg, double* lossh_sum, double* lossh_sumsq);
int  hpf_branch_stats_end(hpf_handle* h);

/* Voltage waveforms: the time-domain voltage v(t) of every bus over one fundamental period, on the device -- its peak (insulation and capacitor
 * stress) and crest factor, the one family of quantities here that depends on the harmonics' phase angles.  The reference has no counterpart.
 * The handle does not know the harmonic orders: orders [Hn] (int32, 1 <= order <= 32767) come with the call, as for hpf_set_sources.  T = samples
 * per fundamental period, a power of two, 64 <= T <= 4096.  U[i][q] = the rectangular voltage of bus i at harmonic position q (p.u. of the nominal
 * PEAK voltage: |U[i][0]| is the amplitude of the fundamental).
 *   table:   ct[j] = cos(j w), st[j] = sin(j w), w = 6.283185307179586 / T, j < T: the host libm's values of (double)j * w, the quadrant points
 *            j = 0, T/4, T/2, 3T/4 set exactly to 0 and +-1; formed on the host, uploaded (hpf_waveform_table returns the same table)
 *   sample:  k = 0 .. T-1:  j = (orders[q] k) & (T - 1)  (integer phase: no argument reduction),
 *            v[k] = sum_q (U[q].re ct[j] - U[q].im st[j]),  sequentially over ascending q from 0.0; every product, difference and sum rounded on its own
 *   peak  = max_k |v[k]|,  kpeak = its sample, ties to the SMALLEST k (inside a lane and across the wave reduction alike: the result does not
 *           depend on the lane mapping); a NaN sample is the peak (numpy's max / argmax)
 *   rms   = sqrt(0.5 s),  s = sum_q (U[q].re^2 + U[q].im^2) sequentially over ascending q
 *   crest = peak / rms, formed as 1.4142135623730951 * (peak / sqrt(s)): sqrt 2 to the last bit for a pure sine of any amplitude (peak / sqrt(0.5 s)
 *           misses that by an ulp for amplitudes such as 1.0); NaN or inf where s = 0
 *   slack = (0.5 (pi/T)^2) sum_q orders[q]^2 |U[q]|,  |U| = sqrt(re^2 + im^2), pi = 3.141592653589793: the continuous peak lies in
 *           [peak, peak + slack]  (at a true maximum v' = 0 and |v''| <= sum h^2 |U|)
 * One wavefront per (scenario, bus) evaluates the T samples from the table in LDS (k_wave_peaks); no atomics.
 * hpf_waveform_table: host only; HPF_E_ARG for a bad T or a NULL pointer.
 * hpf_waveform: evaluates at the handle's CURRENT STATE under the rules of hpf_branch_flows (after hpf_solve, or after hpf_set_state alone: the
 *   rectangular voltages are refreshed from the state first); every solver.  sel [n_sel]: bus indices whose samples go to v [S][n_sel][T], in the
 *   caller's order (n_sel may be 0, v may be NULL).  peak, crest, slack [S][n] double, kpeak [S][n] int32; any of them may be NULL.  HPF_E_ARG,
 *   checked on the host first, for a bad T, an order outside 1 .. 32767, a sel entry outside 0 .. n-1; HPF_E_STATE without a batch.
 * Waveform statistics of a sweep (the third accumulator beside hpf_distortion_* and hpf_branch_stats_*: same state rules, same scenario lists, same
 *   rule for who is added / skipped / deferred, same ids through "distortion_id_base"): per bus the peak against peak_limit[i] and the crest factor
 *   against crest_limit.  k_wave_peaks writes both into a per-handle scratch [max_scenarios][n], one thread per bus folds them (k_wave_add, launched
 *   where k_branch_add is -- every solver, the queue's harvest rounds, the waves of dense / meshed / pivoted handles): max, arg, over and counts do
 *   not depend on slot count, queue chunk, scenario groups or number of GPUs; the four sum arrays do by rounding alone.  Closed (the default):
 *   nothing is allocated or launched, every output of every entry point is unchanged; open: records and voltages are unchanged too (it only reads).
 * hpf_waveform_stats_begin: allocate, zero, open (on an open one: reset).  peak_limit [n] (NULL: +inf); HPF_E_ARG for a NaN limit, a bad T or order.
 * hpf_waveform_stats_add: fold the current batch in, scenario s under id first_id + s (first_id >= 0); HPF_E_STATE unless hpf_solve was the last
 *   call that touched the batch, or with the accumulator closed.
 * hpf_waveform_stats_get: copies out whichever arrays are non-NULL; leaves the accumulator open.  HPF_E_STATE when closed.
 *   counts [3] int64: scenarios added, skipped, deferred
 *   peak_max [n] double, peak_arg [n] int32 (ties: the smallest id; 0 / -1 before the first add), peak_sum, peak_sumsq [n] double,
 *   peak_over [n] uint32: scenarios with peak[i] > peak_limit[i] (strictly);  crest_max .. crest_over: the same five against crest_limit
 * hpf_waveform_stats_end: free (HPF_OK when already closed: a begin / end pair leaves hpf_debug_device_memory as it was); hpf_destroy frees an open
 *   one.  All of them: HPF_E_ARG for a NULL handle, before any HIP call. */
int  hpf_waveform_table(int T, double* ct, double* st);
int  hpf_waveform(hpf_handle* h, const int32_t* orders, int T, int n_sel, const int32_t* sel, double* v, double* peak, int32_t* kpeak,
                  double* crest, double* slack);
int  hpf_waveform_stats_begin(hpf_handle* h, const int32_t* orders, int T, const double* peak_limit, double crest_limit);
int  hpf_waveform_stats_add(hpf_handle* h, int first_id);
int  hpf_waveform_stats_get(hpf_handle* h, int64_t* counts, double* peak_max, int32_t* peak_arg, double* peak_sum, double* peak_sumsq,
                            uint32_t* peak_over, double* crest_max, int32_t* crest_arg, double* crest_sum, double* crest_sumsq,
                            uint32_t* crest_over);
int  hpf_waveform_stats_end(hpf_handle* h);

/* Impedance scan: the driving-point impedances Z_ii(h) = (Y(h)^-1)_ii of every bus, and the transfer columns Z_ij(h) of selected buses j, over a
 * grid of F REAL harmonic orders h > 0 -- where the network resonates.  The reference has no counterpart.  Stateless like hpf_sparse_solve: no
 * handle; the Newton path is not involved.  No matrix is stored: the network is a BFS spanning tree from bus 0 (neighbours in ascending branch
 * index) plus at most HPF_ZSCAN_MAX_TIES loop-closing branches ("ties"), and per frequency point one upward and one downward walk of the tree in
 * complex scalars give the diagonal of the tree's inverse, a walk from bus j its column j, and the ties enter as a rank-k correction
 * (csrc/hpf_zscan.hpp states every recurrence with its association).
 *   net:     n buses, nb branches (from[e] < to[e], 0-based, every pair once: the numbering of hpf_get_branches), series R, X per branch; per bus
 *            gsh, bsh (line-charging halves) and xsh (bus shunt reactance, 0: none)
 *   y_e(h) = 1 / (R_e + j h X_e);  Y_ij = -y_e;
 *   Y_ii   = sum_{e at i} y_e + (gsh_i + j h bsh_i) + [xsh_i != 0 and h != 1] 1 / (j xsh_i h) + y_extra[f][i]
 *            -- the matrix of build_admittance_matrices (HG:147-170) at every real h, its h != 1 rule included
 *   y_extra: [F][n] complex (interleaved re, im) or NULL: caller-supplied shunt admittances per frequency point and bus
 *   sel:     [n_sel] bus indices, 0 <= n_sel <= HPF_ZSCAN_MAX_SEL, whose columns go to Zt [F][n_sel][n] complex (Zt NULL iff n_sel = 0)
 *   Z:       [F][n] complex, may be NULL (peaks only)
 *   zpeak:   [n] max_f |Z_ii|, |z| = sqrt(re^2 + im^2); fpeak [n] int32 its grid index, ties to the smallest f; a NaN is the peak.  Either may be NULL.
 *   chunk:   the grid is processed in chunks of frequency points so that the device scratch stays under 256 MiB (0: automatic, a multiple of 64);
 *            chunk > 0 forces the length.  Every output is bit-identical for every chunk length.
 * One thread per (bus of the current tree depth, frequency point), the frequency fastest; all device arrays are [bus][chunk], so a wavefront
 * reads and writes 64 consecutive complex values; one launch per depth and walk; no atomics.  All device memory is per-call workspace and is
 * released on every return path (hpf_debug_device_memory reads the same before and after).
 * HPF_E_ARG, checked on the host before any HIP call: NULL net or h; n < 1, n > 2^22, nb < 0, F < 1, F > 2^20; a NULL model array; from >= to, an
 * end bus outside 0 .. n-1, a duplicate pair; R = X = 0 on a branch; any non-finite input; h <= 0; n_sel outside 0 .. 64, a sel entry outside
 * 0 .. n-1, Zt NULL with n_sel > 0; chunk < 0, or a forced chunk with n ceil(chunk / 256) > 2^30.  HPF_E_TOPOLOGY (host, too): not connected
 * from bus 0, or more than HPF_ZSCAN_MAX_TIES ties.  HPF_E_SINGULAR, with the outputs still written, when any Z_ii is not finite (a floating
 * network at h = 1, an exact resonance). */
#define HPF_ZSCAN_MAX_TIES 8
#define HPF_ZSCAN_MAX_SEL 64
typedef struct hpf_zscan_net {
    int32_t n, nb;
    const int32_t *from, *to;        /* [nb] */
    const double *R, *X;             /* [nb] */
    const double *gsh, *bsh, *xsh;   /* [n] */
} hpf_zscan_net;
int  hpf_impedance_scan(int device, const hpf_zscan_net* net, int F, const double* h, const double* y_extra, int n_sel, const int32_t* sel,
                        int chunk, double* Z, double* Zt, double* zpeak, int32_t* fpeak);

/* Harmonic penetration ("current injection method"): the bus voltages V(h) = Y(h)^-1 I(h) that S scenarios of injected harmonic currents produce,
 * over a grid of F REAL harmonic orders h > 0, with statistics over the scenarios.  The reference has no counterpart.  Stateless like
 * hpf_impedance_scan: no handle; the Newton path is not involved.  net, h, y_extra, Y(h), the spanning tree and the ties are those of
 * hpf_impedance_scan; the tree factor (w, t, the tie columns, W^-1) is formed once per frequency point by the scan's kernels and shared by all
 * scenarios, and per (point, scenario) one upward and one downward walk of the tree in complex scalars, plus a rank-k correction for k ties, give
 * V (csrc/hpf_penetration.hpp states every recurrence with its association).
 *   inj:     [n_inj] distinct bus indices, 1 <= n_inj <= n: the buses that inject; every other bus injects zero
 *   I:       [S][F][n_inj] complex (interleaved re, im): the current injected INTO the network at bus inj[q], point f, scenario s
 *   V:       [S][F][n] complex, may be NULL (statistics only)
 *   rss:     [S][n] sqrt(sum_f |V|^2) over ALL grid points (leave h = 1 out of the grid for "harmonics only"), may be NULL
 *   vmax, varg (int32), vsum, vsumsq: [F][n], over the scenarios: the maximum of |V|, |v| = sqrt(re^2 + im^2), the scenario it belongs to (ties to
 *            the smallest s; a NaN is the maximum), sum_s |V| and sum_s |V|^2 (sequential over ascending s).  Each may be NULL.
 *   rss_max, rss_arg (int32), rss_sum, rss_sumsq: [n], the same four of rss[s][i] over the scenarios.  Each may be NULL.
 *   chunk_f, chunk_s: the work is cut into chunks of frequency points (outer loop) and scenarios (inner loop), both ascending, so that the device
 *            scratch of a chunk (w, t, the tie columns, W^-1, the right-hand sides and the staging buffer) stays under 256 MiB; 0: automatic, > 0
 *            forces the length.  The carried rss sums [S][n] and the running statistics [F][n] sit outside that budget.  Every output is
 *            bit-identical for every chunking.
 * One thread per (bus of the current tree depth, j = f chunk_s + s), the scenario fastest: the right-hand sides live in place as [bus][j], so a
 * wavefront reads and writes 64 consecutive complex values and one w_i, t_i; one launch per depth and walk; no atomics.  All device memory is
 * per-call workspace and is released on every return path (hpf_debug_device_memory reads the same before and after).
 * HPF_E_ARG, checked on the host before any HIP call: everything hpf_impedance_scan rejects for net, F, h and y_extra; S < 1, S > 2^16; n_inj < 1,
 * n_inj > n; a NULL inj or I; an inj entry outside 0 .. n-1 or one that appears twice; a non-finite entry of I; S n > 2^27; a negative chunk, or
 * forced chunks with n chunk_f chunk_s > 2^30.  HPF_E_TOPOLOGY exactly as hpf_impedance_scan returns it.  HPF_E_SINGULAR, with the outputs still
 * written, when any V is not finite. */
int  hpf_penetration(int device, const hpf_zscan_net* net, int F, const double* h, const double* y_extra, int S, int n_inj, const int32_t* inj,
                     const double* I, int chunk_f, int chunk_s, double* V, double* rss, double* vmax, int32_t* varg, double* vsum, double* vsumsq,
                     double* rss_max, int32_t* rss_arg, double* rss_sum, double* rss_sumsq);

/* Resonance mode analysis: per point of a grid of F REAL harmonic orders h > 0, the eigenvalue of Y(h) of smallest modulus (the critical mode), its
 * modal impedance and the participation factors of the buses -- which resonance the peaks of an impedance scan belong to, and which buses excite
 * and observe it most.  The reference has no counterpart.  Stateless like hpf_impedance_scan: no handle; the Newton path is not involved.  net, h,
 * y_extra, chunk, Y(h), the spanning tree and the ties are those of hpf_impedance_scan; the tree factor (w, t, the tie columns, W^-1) is formed
 * once per frequency point by the scan's kernels, and `iters` steps of inverse iteration run around the right-hand-side walks of hpf_penetration
 * with one scenario (csrc/hpf_resonance.hpp states every recurrence with its association):
 *   x_i = 1 + i / n;   k = 1 .. iters:  y = Y^-1 x,  p = argmax_i |y_i|,  x = y / y_p (not after the last step)
 *   mu = (x . y) / (x . x) without a conjugate (Y is complex symmetric),  lambda = 1 / mu
 *   iters:   1 .. 256 steps, the same at every point; nothing is retried or adapted
 *   lam:     [F] complex (interleaved re, im): the critical eigenvalue
 *   zm:      [F] the critical modal impedance |mu| = 1 / |lambda|, |z| = sqrt(re^2 + im^2)
 *   res:     [F] max_i |x_i - lambda y_i| / (|lambda| |y_p|) = || Y y - lambda y ||_inf / (|lambda| || y ||_inf) of the returned pair: large where
 *            two modes cross or iters is too small -- how a caller knows that a point is not resolved
 *   top:     [F] int32 the bus p of the last step (|y_p| largest, ties to the smallest bus; a NaN is the largest): the largest participation
 *   pf:      [F][n] complex participation factors y_i^2 / (y . y), sum_i pf_i = 1; may be NULL.  Each of lam, zm, res, top may be NULL as well.
 *   chunk:   as for hpf_impedance_scan; the scratch of a chunk (the factor, x, y, pf, the partial maxima and sums, the staging buffer) stays under
 *            256 MiB.  Every output is bit-identical for every chunk length.
 * All device arrays are [bus][chunk] or [tile of 32 buses][chunk], the frequency fastest, so a wavefront reads and writes 64 consecutive values;
 * every reduction over the buses is a partial result per tile and then one thread per point over the tiles, the sums in ascending order; no
 * atomics.  All device memory is per-call workspace and is released on every return path (hpf_debug_device_memory reads the same before and after).
 * HPF_E_ARG, checked on the host before any HIP call: everything hpf_impedance_scan rejects for net, F, h, y_extra and chunk; iters outside
 * 1 .. 256.  HPF_E_TOPOLOGY exactly as hpf_impedance_scan returns it.  HPF_E_SINGULAR, with the outputs still written, when any lam, zm, res or pf
 * is not finite (a singular Y(h): lambda = 0 has no modal impedance). */
int  hpf_resonance_modes(int device, const hpf_zscan_net* net, int F, const double* h, const double* y_extra, int iters, int chunk, double* lam,
                         double* zm, double* res, int32_t* top, double* pf);

/* Start state: warm-start the scenarios of a sweep from one solved case instead of the reference's flat start (HG:174-184) + pf (HG:244-275).  The
 * reference has no counterpart (hpf() always starts flat, HG:511-529).  The scenarios of a Monte-Carlo sweep sit close to each other: from the whole
 * raw state of the feeder solved at its nominal loads the harmonic NR needs 2 - 3 iterations where the flat start needs 20 - 30.
 * The handle owns ONE start state: Vm, Va of one scenario and the U = Vm e^(j Va), E = U / Vm formed from them once (the arithmetic hpf_solve applies
 * to a state set with hpf_set_state), in the bus-major layout of the state.  Unset (the default): nothing is allocated, no kernel is launched, every
 * output of every entry point is unchanged.
 * hpf_start_set: Vm0, Va0 [Hn*n] host arrays in the ABI's stacked order, raw (signed, un-wrapped, as hpf_get_state returns them); replaces a set
 *   one.  HPF_E_ARG for a NULL handle or pointer, a non-finite entry or a zero magnitude (E = U / Vm) -- all checked on the host before any HIP call.
 * hpf_start_capture: the same from scenario `scen` of the current batch, device to device: a base case solved on this handle becomes the start
 *   without a host round trip.  HPF_E_STATE without a batch, HPF_E_ARG for scen outside the batch.  A scenario whose state holds an entry
 *   hpf_start_set would refuse (non-finite, zero magnitude; checked by the kernel) returns HPF_E_STATE; after that, or after a HIP error, the
 *   handle holds NO start state (a set one is lost: its buffers were being overwritten).
 * hpf_start_get: copies the start state out (stacked order); HPF_E_STATE when unset.
 * hpf_start_clear: frees the buffers (HPF_OK when already unset); hpf_destroy frees a set one.
 * hpf_start_apply: = hpf_set_state of the start state tiled to n_scen scenarios, broadcast on the device (the argument rules of hpf_set_state);
 *   HPF_E_STATE when unset.  The handle remembers that the batch came from the start state until the next hpf_set_state: hpf_solve then sets
 *   hpf_stat.flags bit 8.
 * hpf_solve_queue with a start state set: every scenario begins at it and the pf phase is skipped (no pf waves, no seed arrays; thresh_f and
 *   max_iter_f are ignored); radial BLOCK_TREE handles move a new scenario into its storage with the start state instead of the pf seed
 *   (k_queue_init_start), the other handles run hpf_start_apply + hpf_solve per wave.  Every record carries flags bit 8, and a scenario's record and
 *   voltages are bit-identical to hpf_start_apply(1) + hpf_set_loads + hpf_solve alone, whatever the slot count, "queue_chunk" or "scenario_groups".
 *   Flags bits 2, 3 and 6 keep their meaning: hpf_solve repeats a flagged batch from the state the call was entered with, i.e. the start state.
 *   A started scenario that does NOT converge (hit max_iter, non-finite) is reported with bit 8 and its usual bits; the caller solves it again from
 *   the reference's start.  For the distortion accumulator and the branch statistics such a scenario (bit 8 set, bit 0 clear) counts as DEFERRED, not
 *   skipped, so that this re-solve adds it exactly once. */
int  hpf_start_set(hpf_handle* h, const double* Vm0, const double* Va0);
int  hpf_start_capture(hpf_handle* h, int scen);
int  hpf_start_get(hpf_handle* h, double* Vm0, double* Va0);
int  hpf_start_clear(hpf_handle* h);
int  hpf_start_apply(hpf_handle* h, int n_scen);

/* Source currents: per-scenario Norton source currents, the quantity a probabilistic harmonic study randomises (how many units of a device are in
 * service, and the phase-angle diversity between devices that decides their cancellation).  The reference has no counterpart: its Norton data are
 * per device type (HG:278-310).  A nonlinear bus i (m <= i < n) has current-balance rows only, I_inj = I_N - Y_N U (HG:313-323, 347-354); with sources
 * set, scenario s forms them with I_src[s][i - m][q] in place of I_N[dev(i)][q] at every harmonic position q.  Y_N stays the model's: the Jacobian,
 * the tree plan and every per-model image are untouched, only the right-hand side of the Newton step changes.
 * Two input forms (`form`):
 *   HPF_SRC_CURRENTS (0): data = I_src itself, [S][n - m][Hn] complex (interleaved re, im), p.u.; used as given.
 *   HPF_SRC_SCALE_SHIFT (1): data = (a, phi) [S][n - m][2] doubles -- a units of the bus's device, their waveform shifted in time by phi radians at
 *     the fundamental, so that harmonic order h rotates by h phi: I_src[q] = (a e^(j h_q phi)) I_N[dev(i)][q].  The handle does not know the harmonic
 *     orders: orders [Hn] (1, 3, 5, ...) comes with the data.  Expanded on the device (k_source_expand) with the rounding of csrc/hpf_sources.hpp:
 *     ang = (double)h_q * phi; (s, c) = sincos(ang); w = (a c, a s); I = (w.re in.re - w.im in.im, w.re in.im + w.im in.re), every product and sum
 *     rounded on its own.
 * Sources belong to the batch's LOADS.  hpf_set_sources needs a batch with loads (HPF_E_STATE otherwise) and n_scen == hpf_num_scenarios (else
 *   HPF_E_ARG); hpf_set_loads DROPS them -- the next mismatch uses the model's I_N again, so no source leaks into another batch.  hpf_set_state and
 *   hpf_start_apply keep them.
 * Argument checks, all on the host before any HIP call, HPF_E_ARG: a NULL handle or NULL data, an unknown form, orders NULL with form 1, n_scen < 1,
 *   a non-finite entry.  A model without nonlinear buses (m == n): HPF_OK, nothing is done.
 * hpf_get_sources: the I_src the device holds for the batch, [S][n - m][Hn] complex (after form 1: the expanded currents).  HPF_E_STATE when the
 *   batch has none (never set, cleared, or dropped by hpf_set_loads).
 * hpf_clear_sources: the batch goes back to the model's I_N; frees the storage and a pending registration (HPF_OK when there is none); hpf_destroy
 *   frees them too.  On a batch WITH sources it ends the mismatch and "hpf_solve was the last call" like hpf_set_sources does; on a batch without
 *   (never set, or dropped by hpf_set_loads) it changes nothing of the batch, whatever storage it frees.
 * hpf_queue_sources: the sources of a whole sweep of n_total scenarios (same forms, [n_total][...]), uploaded to HBM and consumed by the NEXT
 *   hpf_solve_queue.  If that call's n_total differs it returns HPF_E_ARG, the registration is dropped and nothing is solved.  Radial BLOCK_TREE
 *   handles move a scenario's sources into its storage with its loads (k_source_gather / k_source_expand next to k_queue_init); the wave handles
 *   (DENSE, meshed, pivoted) set each wave's sources device to device after its loads.  A scenario's record and voltages are bit-identical to
 *   hpf_set_loads + hpf_set_sources + (hpf_fund_pf) + hpf_solve of that scenario alone, whatever the slot count, "queue_chunk" or
 *   "scenario_groups".  Afterwards the handle holds no batch and no sources.
 * What sees the sources: hpf_mismatch, hpf_solve (its pivoted repeat and the trace included), hpf_solve_queue, hpf_iterate, the step-residual check,
 *   both update modes.  NOT affected: hpf_fund_mismatch / hpf_fund_pf (the fundamental pf uses P, Q only), the Jacobian entry points, the start
 *   state, the accumulators (they read voltages).  Records of scenarios solved with sources carry hpf_stat.flags bit 10.
 * Unset (the default): nothing is allocated, no launch is added or changed (the kernels' source variants are separate instantiations), every output
 *   of every entry point is bit-identical. */
enum { HPF_SRC_CURRENTS = 0, HPF_SRC_SCALE_SHIFT = 1 };
int  hpf_set_sources(hpf_handle* h, int n_scen, int form, const double* data, const int32_t* orders);
int  hpf_get_sources(hpf_handle* h, double* I_src /* [S][n-m][Hn] complex, as the device holds them */);
int  hpf_clear_sources(hpf_handle* h);
int  hpf_queue_sources(hpf_handle* h, int n_total, int form, const double* data, const int32_t* orders);

/* Diagnostics: with env HPF_DEBUG_ABLATE & 16 the BLOCK_TREE factor kernel records shader-cycle stamps per (scenario, bus):
 * out[(s*n + k)*8 + 0..5] = assembly, packed sub-phases, packed Gauss-Jordan split, MFMA Gauss-Jordan, packed wave-0 roles,
 * Schur push (tools/stamps.py decodes them; -DHPF_FACTOR_STAMPS build only); [6] dense children,
 * [7] nonlinear bus.  Timing-only; never read by any kernel. */
int  hpf_debug_stamps(hpf_handle* h, long long* out, int count);

/* Diagnostics: device blocks and bytes the library holds at this moment, over all handles and running calls of the process (its own
 * bookkeeping: every block it allocates has one owner, and the owners count; the per-call workspace of hpf_sparse_solve is not included).
 * Either argument may be null.  After the last hpf_destroy both are 0; a begin / end pair (hpf_distortion_*, hpf_branch_stats_*,
 * hpf_start_set / _clear, hpf_set_sources / hpf_clear_sources) leaves both as they were.  Unlike the device's free memory the figures do
 * not depend on what else runs on the device, so a test can assert them exactly.  Always HPF_OK. */
int  hpf_debug_device_memory(int64_t* blocks, int64_t* bytes);

/* Options.  "block_pivoting" (BLOCK_TREE only): 0 (default) inverts the 2Hn x 2Hn bus blocks on the FP64 matrix cores with
 * a static pivot order (4x4 blocks = two harmonics, lane-parallel cofactor inverse), after contracting pass-through buses and
 * with per-model constant inverses for nonlinear leaf buses; 1 uses wave-level Gauss-Jordan with partial pivoting over the
 * whole block on the uncontracted tree (slower, for networks whose bus blocks are not block-diagonally dominant).  Env
 * HPF_GJ_MODE=0 selects the pivoted variant process-wide.  Changing the value ends a valid mismatch (the two variants read it in different
 * layouts): hpf_mismatch again before hpf_iterate.  Meshed handles: 1 is refused with HPF_E_STATE.
 * "pivot_growth_limit_log10" (0..300, default 10): the static-pivot monitor flags a scenario when |a_ij W_ji| of a pivot block
 * (a lower bound of its condition number) exceeds 10^value; "auto_repivot" (default 1): hpf_solve repeats flagged scenarios
 * with partial pivoting (0: they are only reported in hpf_stat.flags).
 * "keep_previous_state" (default 0): hpf_solve keeps per scenario the state its last Newton step started from (hpf_jacobian_last).
 * "border_pivoting" (meshed BLOCK_TREE handles, default 0): the m x m border system of a bordered Newton step is factored WITHOUT pivoting
 * first (rocSOLVER's pivoted LU spends a third of such a step in tiny pivot-search kernels) and its solution checked against a kept copy of
 * the system; a relative residual above 1e-10, a zero pivot or a non-finite entry repeats it with partial pivoting (hpf_tree_census[11]
 * counts those).  1 = always the pivoted LU.
 * "queue_chunk" (1..16, default 4): Newton iterations between two harvest / refill rounds of hpf_solve_queue.
 * "step_residual_check" (0 / 1, default 0): after the linear solve of every harmonic Newton step -- hpf_solve, hpf_solve_queue, hpf_iterate; every
 * solver and path -- one more pass over the assembly forms r = f - J dx row by row without storing J (the entries of hpf_jacobian_csr) and the
 * scenario's normwise backward error eta (hpf_get_step_residuals).  A step with eta above 10^"step_residual_limit_log10" (-16..0, default -10:
 * healthy steps of every path sit below 1e-12, the evaluation's own rounding below 2e-14) or a non-finite eta sets hpf_stat.flags bit 6; hpf_solve
 * treats the scenario like one flagged by the static-pivot monitor (repeat with partial pivoting where that exists, "auto_repivot"; the check runs
 * in the repeat too and bit 7 is the verdict on the pass whose result is returned).  Off: no launch is added, results are bit-identical.
 * "rectangular_update" (0 / 1, default 0; any other value: HPF_E_ARG): how a harmonic Newton step dx = (dtheta, dV) of J dx = f moves the state.  0: the
 * reference's update, added to (Va, Vm) (HG:478,484-485).  1: in rectangular coordinates, where the step is exact for every row that is linear in
 * U = Vm e^(j Va) (all current-balance rows): for entry (bus i, harmonic position q), k = q n + i, with vm, va its state and u, e the U, E the handle
 * holds for it (E = U / Vm),
 *   k <  c (slack, PV fundamentals: the magnitude is no state variable): the reference's update, unchanged;
 *   k >= c: b = vm dtheta,  dU = (e.re dV - e.im b, e.re b + e.im dV),  U' = u - dU,  vm' = sqrt(U'.re^2 + U'.im^2),  va' = atan2(U'.im, U'.re)
 * (csrc/hpf_update.hpp; every product and sum rounded on its own; vm may be negative, vm' never is; U' = 0: vm' = 0, va' = 0).  The stored U, E are
 * then formed from (vm', va') like after every update and hpf_set_state, NOT taken from U' (at vm' = 0: U = 0, E = 1).  From the reference's start
 * the harmonic NR then needs 3 - 4 iterations where the reference's update needs 20 - 30; the fixed point is the same, the iterates
 * and the last digits of the result are not.  One site serves hpf_solve (its pivoted repeat and the trace included), hpf_solve_queue (chunks and
 * waves) and hpf_iterate, every solver; the fundamental pf (hpf_fund_pf) keeps the reference's update.  May be changed between calls: takes effect
 * at the next hpf_solve / hpf_solve_queue / hpf_iterate.  Records of scenarios solved with it carry hpf_stat.flags bit 9.  A scenario with bit 9
 * that does NOT converge (bit 0 clear) is solved again by the caller with the option off; for the distortion accumulator and the branch statistics
 * it counts as DEFERRED, not skipped (like bit 8), so that this re-solve adds it exactly once.  Off: no launch is added or changed, every output of
 * every entry point is bit-identical.
 * "distortion_id_base" (>= 0, default 0): with the distortion accumulator or the branch statistics open (it serves both), hpf_solve_queue adds
 * scenario g of a call under id value + g.
 * "scenario_groups" (1..8, default 4; at least 32 running scenarios per group): independent scenario pipelines on separate HIP streams -- group 0
 * on the handle's own stream (hpf_set_stream), the others on streams of the handle.  The runtime maps streams onto FOUR hardware queues: with a fifth
 * stream busy at the same time (the application's own work during a solve) two groups share a queue and serialise (1.25 instead of 0.90 ms per
 * step at the benchmark shape) -- such an application sets 3.
 * Switches read by hpf_create (diagnostics, A/B runs; from the option string of hpf_create_opts -- the first occurrence of a name counts --, and
 * from the environment only with HPF_ENV_SWITCHES=1; HPF_HOST_THREADS -- host threads of the tree planner, no effect on results -- is always read
 * from the environment; HPF_TREE_DUMP takes a path: environment only, ignored in an option string; the one list of them with their defaults is
 * struct hpf::Switches in csrc/hpf_switches.hpp): HPF_DEBUG_ABLATE (timing-only ablation of factor-kernel phases: results INVALID), HPF_GJ_MODE=0
 * (the pivoted variant for every solve of the handle), HPF_LAZY=0 builds the elimination tree without lazy leaves (every
 * leaf writes its Schur complement; 1: only leaves directly under their dense parent), HPF_SLEAF=0 sends the nonlinear buses
 * whose dense children are all lazy leaves (super-leaves: bordered low-rank inverse) through Gauss-Jordan like every other bus,
 * HPF_LEAFBATCH=0 runs the lazy leaves one workgroup per (leaf, scenario) instead of 16 scenarios per workgroup on the matrix
 * cores, HPF_SLBACK=0 lets the super-leaves store their inverse for the per-scenario back sweep instead of keeping T^-1 only,
 * HPF_SLLAZY=0 lets every super-leaf push its Schur complement itself (no vector-only bordered buses, hence no nested ones: the
 * faster build up to about 24 live scenarios), HPF_SLNEST=0 keeps bordered buses below bordered buses on the
 * Gauss-Jordan path, HPF_FUSELEVEL=0 launches the scenario-batched
 * and the per-scenario workgroups of an elimination level separately (k_leaf_batch / k_sleaf_batch + k_factor_q instead of k_level),
 * HPF_LINBUNDLE=0 / HPF_LINTREE=0 run the 2x2 algebra of the linear subtrees height by height in one launch / in one launch per
 * height, HPF_CHAINBUNDLE=0 gives the contracted chains their own launches, HPF_COMPRESS=0 eliminates the Gauss-Jordan buses strictly
 * leaves first (no compress steps: one elimination level per unit of tree height; 5 - 8 % faster per step from about 384 live scenarios on, whose
 * levels fill the chip -- the steps are the default at every capacity so that a handle's Newton steps do not depend on its capacity), HPF_TREE_INFO=1 prints the tree statistics to stderr,
 * HPF_QUEUE_INFO=1 prints the phase times of hpf_solve_queue to stderr, HPF_BORDER_SLOTS=n caps the virtual scenario slots a meshed handle
 * allocates for its bordered step (default 1 024, at least 16: the m + 1 right-hand sides run in chunks of that many; only with HPF_MESH_SEL=0),
 * HPF_MESH_SEL=0 runs the bordered step of a meshed handle in its form of rounds 2 - 4 (the m unit right-hand sides as virtual scenarios through
 * the tree kernels, the tree re-factorised for each) instead of the factor-once form (one sweep + a selected inversion over the tie endpoints'
 * root paths, whose buses the planner then keeps as plain Gauss-Jordan buses; coupled models), HPF_MESH_BATCH_GB=x bounds the memory of
 * the per-scenario buffers of that form (default 48, and not more than half of the device's free memory: as many scenarios per batch as fit, at least one), HPF_BORDER_GJ=n solves border systems of up to n endpoint buses (default 96) by a
 * block Gauss-Jordan elimination with the library's own block-product kernel and larger ones by rocSOLVER's LU (0: always rocSOLVER;
 * HPF_BORDER_GJ_MFMA=0 inverts its diagonal blocks on the vector units instead of the matrix cores, HPF_BORDER_PIVLIM=x sets the amplification of
 * a 4 x 4 pivot block beyond which such a system goes to the pivoted LU, default 1e3; HPF_BORDER_INFO=1 prints every border solve's residual),
 * HPF_FUSEBACK=0 launches the back sweep's scenario-batched workgroups (bordered buses, leaves) after the last depth instead of inside the
 * depths' launches (k_level_back: groups of up to HPF_FUSEBACK_MAX = 32 scenarios, blocks of 52),
 * HPF_BATCH_TILE8_MAX=n lets the factor sweep's batched bordered buses take 8 scenarios per workgroup (32 threads per scenario) instead of 16 in
 * scenario groups of up to n (default 32; 0: never), HPF_LEAF_TILE8_MAX=n the same for its lazy leaves (default 0); the results are the same bits,
 * HPF_BACKWALK=0 runs the back sweep's Gauss-Jordan buses in one launch per depth instead of two tree walks (k_back_walk: the trunk,
 * then up to 8 subtree lists, one workgroup per list and scenario; blocks of 52, groups of HPF_BACKWALK_MIN = 16 to HPF_BACKWALK_MAX = 256
 * scenarios: groups of 1 - 4 run faster on the depth launches; the batched workgroups follow the walk),
 * HPF_BACKTAIL=0 runs those batched workgroups, wherever they follow the Gauss-Jordan buses, in one launch per nesting order of the bordered
 * buses and one for the leaves instead of one launch (k_back_tail: one workgroup per family -- a bordered bus under a Gauss-Jordan bus, its nested
 * bordered buses and their leaves -- and 16 scenarios, the x of a member's parent kept in LDS),
 * HPF_GROUPS=n presets "scenario_groups".  Every switch selects a path with the same Newton steps (tests/test_gpu_robustness.py). */
int  hpf_set_option(hpf_handle* h, const char* name, int value);

/* Stream plumbing: run on a caller stream (e.g. torch's current stream) instead of the handle's own; NULL restores. */
int  hpf_set_stream(hpf_handle* h, void* hip_stream);
int  hpf_sync(hpf_handle* h);

/* Kernel timing with HIP events on the handle's stream, accumulated since the last reset.
 * which: 0 mismatch kernel, 1 Jacobian assembly kernels (DENSE only; BLOCK_TREE assembles inside the factor kernel),
 * 2 linear solve (DENSE: getrf+getrs, one span per step; BLOCK_TREE: one span per launch of a factor kernel OTHER than the
 *   general one: k_leaf_batch, k_sleaf_batch, the leaf-only k_factor_q<B,true>, the pivoted / generic kernels),
 * 3 state update, 4 back-substitution sweep (BLOCK_TREE only; one span per Newton step and scenario group),
 * 5 BLOCK_TREE: one span per launch of the dominant factor kernel: k_level<B> (b <= 52: one launch per elimination level, every dense bus)
 *   where hpf_tree_census reports fused levels, else the general kernel k_factor_q<B,false>,
 * 6 the same launches on the DEVICE clock: last workgroup end - first workgroup start (wall_clock64 stamps written by the kernel
 *   while timing is enabled) -- what rocprofv3 --kernel-trace reports as the kernel's duration; a HIP-event span additionally
 *   holds the event packets and the queue gaps around a ~25 us kernel.
 * 7 the residual check of the steps (k_step_residual + k_step_eta, option "step_residual_check"; one span per Newton step and scenario group).
 * Returns total milliseconds in *ms and the number of timed spans in *launches. */
int  hpf_timing_enable(hpf_handle* h, int on);   /* 1: HIP-event spans (classes 0..5) + device stamps (6); 2: device stamps only --
                                                    no event packets between the kernels, the launches run exactly as untimed; 0: off */
int  hpf_timing_get(hpf_handle* h, int which, double* ms, int64_t* launches);
int  hpf_timing_reset(hpf_handle* h);
/* FP64 flop count of the span `which == 2` for ONE scenario and ONE Newton step (roofline numerator):
 * DENSE 2/3 N^3 + 2 N^2; BLOCK_TREE (b = 2 Hn) per Gauss-Jordan bus 2 b^3 + 2 b^2 + b^2 per dense child (+ 8 b^2 non-root),
 * per constant-inverse leaf 10 b^2 (+ 8 b^2 push unless lazy: then only G w), per lazy leaf 4 b^2 + 4 b^2 per parent for the
 * rebuild, per super-leaf (m = 2 + 2 L border unknowns) 2 m^3 + 8 b^2 ceil(m/4) + 6 b^2 + 6 b m. */
double hpf_solve_flops(const hpf_handle* h);
/* Algorithmic HBM bytes of the same span (one scenario, one Newton step): BLOCK_TREE every Schur complement once out and once
 * in (lazy leaves: 2x2 core + G w instead), every Gauss-Jordan / super-leaf inverse once out, per-scenario bus operands; DENSE
 * the Jacobian out and through getrf. */
double hpf_solve_bytes(const hpf_handle* h);
/* ... and of the span `which == 4` (BLOCK_TREE back sweep: Gauss-Jordan inverses in, w, A(k,parent), x in / out); 0 for DENSE. */
double hpf_back_bytes(const hpf_handle* h);
/* Roofline model of ONE kernel class (timing span `which`, see hpf_timing_get): algorithmic HBM bytes and FP64 flops of all its
 * launches of one Newton step for ONE scenario, and the number of launches per step and scenario group.  which == 5: the
 * general multi-wave factor kernel k_factor_q<B,false> alone (Gauss-Jordan buses, non-batched super-leaves; the buses of the
 * scenario-batched kernels k_leaf_batch / k_sleaf_batch and of the leaf-only instantiation are NOT in it); which == 2: the
 * whole factor sweep (= hpf_solve_bytes / hpf_solve_flops); which == 4: the back sweep; which == 7 (every solver): the residual check of
 * a step.  Other classes: HPF_E_ARG. */
int  hpf_kernel_model(const hpf_handle* h, int which, double* bytes, double* flops, int* launches);
/* Census of the BLOCK_TREE elimination tree (diagnostic; which kernel takes which bus).  counts[0..8]: buses with a dense b x b
 * block (the rest lives in the 2x2 algebra of the linear subtrees / contracted chains), Gauss-Jordan buses (k_factor_q<B,false>),
 * constant-inverse leaves, of which lazy (vector-only, k_leaf_batch), bordered buses (super-leaves, m x m core), of which nested
 * (bordered children below them), elimination levels, back-sweep depths, tie lines of a meshed network, [9] 1 if every elimination
 * level is ONE launch (k_level: scenario-batched and per-scenario workgroups in one grid; timing class 5 then covers it) -- blocks of 52
 * in the default mode; smaller blocks only when every level has scenario-batched workgroups (levels without them run k_factor_q's own grid),
 * [10] compress steps (Gauss-Jordan buses eliminated before their tallest dense child: levels counts the shortened chain),
 * [11] border systems of a meshed network that were repeated with the pivoted LU since hpf_create (option "border_pivoting"),
 * [12] border unknowns of a meshed network (2 Hn x distinct endpoint buses of the loop-closing lines), [13] buses on the endpoints' root paths
 * (kept as plain Gauss-Jordan buses by the factor-once bordered step; 0: virtual-sweep form), [14] form of the bordered step: 0 virtual sweeps,
 * 1 factor-once with rocSOLVER's LU of the border system, 2 factor-once with the block Gauss-Jordan solve, [15] back sweeps (scenario group x
 * Newton step) since hpf_create whose Gauss-Jordan buses went through the tree walk (HPF_BACKWALK), [16] back sweeps since hpf_create whose
 * bordered buses and constant-inverse leaves went through one launch that walks their families (k_back_tail, HPF_BACKTAIL),
 * [17] scenarios per batched workgroup of the last factor launch with bordered buses: 16, or 8 where the scenario group is no larger than
 * HPF_BATCH_TILE8_MAX (0: no such launch yet), [18] the same of the last factor launch with lazy leaves (HPF_LEAF_TILE8_MAX).
 * HPF_E_STATE for DENSE. */
int  hpf_tree_census(const hpf_handle* h, int* counts, int n_counts);
/* Wall-clock milliseconds hpf_create spent: ms[0] total, [1] planning the elimination trees on the host (classification of the buses,
 * per-model constant images: complex inversions on host threads, env HPF_HOST_THREADS), [2] uploading them, [3] allocating the
 * per-scenario state.  (The host-side ingest and admittance build happen before hpf_create, in the Python layer.) */
int  hpf_setup_times(const hpf_handle* h, double* ms, int n_ms);
/* Number of scenario groups (independent pipelines on separate HIP streams) a Newton step of `live` running scenarios is split into:
 * option "scenario_groups" bounded by a minimum group size; 1 for DENSE and for meshed networks. */
int  hpf_scenario_groups(const hpf_handle* h, int live);
/* Host-only planning run of the BLOCK_TREE elimination tree of a model (no device is touched, no handle, the process environment
 * is not modified): builds the contracted tree exactly as hpf_create would for a handle of d->max_scenarios scenarios (compress steps
 * are the default) and writes one line per dense bus (bus, dense parent, elimination level, back-sweep depth, kind, ...)
 * to `path` (replaced if it exists; tools/tree_plan.py reads it).  Returns the planning status: HPF_OK when the plan was written,
 * HPF_E_TOPOLOGY as hpf_create would return it, HPF_E_ARG when the file cannot be written.  A meshed model (spanning tree + loop-closing lines):
 * a comment line with the lines / endpoint buses / border size, and a last column that marks the buses on the endpoints' root paths, which the
 * factor-once bordered step keeps as plain Gauss-Jordan buses (1; -1 would be a planner fault).  (env HPF_TREE_DUMP=<file> makes hpf_create itself
 * write the same dump.) */
int  hpf_tree_plan(const hpf_desc* d, const char* path);

#ifdef __cplusplus
}
#endif
#endif /* HPF_H */
