// Build switches of a handle (A/B runs, diagnostics: "HPF_LAZY=0 HPF_SLEAF=1 ..."): the one list of every switch libhpf reads, with its
// default, and their parser.  Plain C++ (no HIP): the host tests compile it on its own.
#pragma once
#include <stdlib.h>
#include <string.h>

#include <string>

namespace hpf {

struct Switches {
    // diagnostics: presence-only (any value, "=0" included, turns them on) ...
    bool tree_info = false;           // HPF_TREE_INFO: tree statistics to stderr
    bool border_info = false;         // HPF_BORDER_INFO: every border solve's residual to stderr
    bool queue_info = false;          // HPF_QUEUE_INFO: phase times of hpf_solve_queue to stderr
    std::string tree_dump;            // HPF_TREE_DUMP: file of the planner's dump (environment only; empty: none)
    int debug_ablate = 0;             // HPF_DEBUG_ABLATE: timing-only ablation of factor-kernel phases (results invalid)
    // the handle
    int gj_mode = 1;                  // HPF_GJ_MODE: initial hpf_handle::gj_mode (0: the pivoted variant for every solve)
    int n_groups = 4;                 // HPF_GROUPS (clamped to 1..8): initial hpf_handle::n_groups ("scenario_groups")
    bool leafbatch = true;            // HPF_LEAFBATCH=0: one workgroup per (leaf, scenario) instead of 16 scenarios per workgroup
    bool fuse_levels = true;          // HPF_FUSELEVEL=0: separate launches for the batched and the per-scenario workgroups of a level
    bool fuse_back = true;            // HPF_FUSEBACK=0: the back sweep's batched launches after the last depth instead of inside the depths' launches
    int fuse_back_max = 32;           // HPF_FUSEBACK_MAX: largest scenario group that takes the fused back sweep
    int batch_tile8_max = 32;         // HPF_BATCH_TILE8_MAX: largest scenario group whose batched bordered buses take tiles of 8 scenarios (32 threads per
                                      // scenario) instead of 16 in the factor sweep; 0: never (measured: a gain up to 32, a loss from 64)
    int leaf_tile8_max = 0;           // HPF_LEAF_TILE8_MAX: the same bound for the lazy leaves of level 0 (their launch is the widest of the sweep: level 0
                                      // of a group of 32 takes 30 us with tiles of 8 against 24 - 26 with tiles of 16)
    bool back_walk = true;            // HPF_BACKWALK=0: the Gauss-Jordan buses of the back sweep in one launch per depth instead of two tree walks
    int back_walk_min = 16;           // HPF_BACKWALK_MIN: smallest scenario group that takes the tree walk (at 1 - 4 its serial per-bus steps lose
                                      // ~8 % of the step to the few short depth launches; at 16 the two tie)
    int back_walk_max = 256;          // HPF_BACKWALK_MAX: largest scenario group that takes the tree walk (measured up to 256: a tie above 32)
    bool back_tail = true;            // HPF_BACKTAIL=0: the batched back sweep behind the walk in one launch per nesting order of the bordered buses and one for
                                      // the leaves instead of one launch that walks their families (k_back_tail)
    int border_slot_cap = 1024;       // HPF_BORDER_SLOTS: cap of the virtual scenario slots of a meshed handle's bordered step
    // the tree planner
    bool lintree = true;              // HPF_LINTREE=0: the 2x2 algebra of the linear subtrees in one launch per height
    bool linbundle = true;            // HPF_LINBUNDLE=0: ... in one launch for every height (no one-round-trip bundles)
    bool chainbundle = true;          // HPF_CHAINBUNDLE=0: the contracted chains get their own launches
    int sleaf = 2;                    // HPF_SLEAF: 0 no super-leaves, 1 nonlinear buses only
    bool slback = true;               // HPF_SLBACK=0: super-leaves store their inverse for the per-scenario back sweep
    bool sllazy = true;               // HPF_SLLAZY=0: every super-leaf pushes its Schur complement itself
    bool slnest = true;               // HPF_SLNEST=0: bordered buses below a bordered bus stay on the Gauss-Jordan path
    int lazy = 2;                     // HPF_LAZY: 0 no lazy leaves, 1 only leaves directly under their dense parent
    bool compress = true;             // HPF_COMPRESS=0: no compress steps
    // meshed networks
    bool mesh_sel = true;             // HPF_MESH_SEL=0: the bordered step with m virtual sweeps instead of the factor-once form
    int border_gj = 96;               // HPF_BORDER_GJ: largest border system (endpoint buses) solved by block Gauss-Jordan
    bool border_gj_mfma = true;       // HPF_BORDER_GJ_MFMA=0: its diagonal blocks inverted on the vector units
    double border_pivlim = 1e3;       // HPF_BORDER_PIVLIM (> 0): pivot-block amplification beyond which a border system goes to the pivoted LU
    double mesh_batch_gb = 48.0;      // HPF_MESH_BATCH_GB: memory bound of the factor-once form's per-scenario buffers ...
    bool mesh_batch_gb_given = false; // ... not capped at half of the free device memory when the switch is given
};

// Each switch is a token NAME=value of `options`, starting the string or following ' ', ',' or ';'; the first occurrence counts.  A name the
// string lacks is read from the environment only when env_opt_in (HPF_ENV_SWITCHES=1).  Values convert with atoi / atof; unknown names are ignored.
inline Switches parse_switches(const char* options, bool env_opt_in) {
    const std::string opts = options ? options : "";
    auto find = [&](const char* name) -> const char* {         // (atoi / atof stop at the separator)
        const size_t ln = strlen(name);
        size_t pos = 0;
        while ((pos = opts.find(name, pos)) != std::string::npos) {
            const bool starts = pos == 0 || opts[pos - 1] == ' ' || opts[pos - 1] == ',' || opts[pos - 1] == ';';
            if (starts && pos + ln < opts.size() && opts[pos + ln] == '=') return opts.c_str() + pos + ln + 1;
            pos += ln;
        }
        return env_opt_in ? getenv(name) : nullptr;
    };
    auto flag = [&](const char* name, bool& f) {
        if (const char* v = find(name)) f = atoi(v) != 0;
    };
    auto integer = [&](const char* name, int& f) {
        if (const char* v = find(name)) f = atoi(v);
    };
    Switches s;
    s.tree_info = find("HPF_TREE_INFO") != nullptr;
    s.border_info = find("HPF_BORDER_INFO") != nullptr;
    s.queue_info = find("HPF_QUEUE_INFO") != nullptr;
    if (env_opt_in)
        if (const char* v = getenv("HPF_TREE_DUMP")) s.tree_dump = v;
    integer("HPF_DEBUG_ABLATE", s.debug_ablate);
    if (const char* v = find("HPF_GJ_MODE")) s.gj_mode = atoi(v) ? 1 : 0;
    if (const char* v = find("HPF_GROUPS")) s.n_groups = atoi(v) < 1 ? 1 : (atoi(v) > 8 ? 8 : atoi(v));
    flag("HPF_LEAFBATCH", s.leafbatch);
    flag("HPF_FUSELEVEL", s.fuse_levels);
    flag("HPF_FUSEBACK", s.fuse_back);
    integer("HPF_FUSEBACK_MAX", s.fuse_back_max);
    integer("HPF_BATCH_TILE8_MAX", s.batch_tile8_max);
    integer("HPF_LEAF_TILE8_MAX", s.leaf_tile8_max);
    flag("HPF_BACKWALK", s.back_walk);
    integer("HPF_BACKWALK_MIN", s.back_walk_min);
    integer("HPF_BACKWALK_MAX", s.back_walk_max);
    flag("HPF_BACKTAIL", s.back_tail);
    integer("HPF_BORDER_SLOTS", s.border_slot_cap);
    flag("HPF_LINTREE", s.lintree);
    flag("HPF_LINBUNDLE", s.linbundle);
    flag("HPF_CHAINBUNDLE", s.chainbundle);
    integer("HPF_SLEAF", s.sleaf);
    flag("HPF_SLBACK", s.slback);
    flag("HPF_SLLAZY", s.sllazy);
    flag("HPF_SLNEST", s.slnest);
    integer("HPF_LAZY", s.lazy);
    flag("HPF_COMPRESS", s.compress);
    flag("HPF_MESH_SEL", s.mesh_sel);
    integer("HPF_BORDER_GJ", s.border_gj);
    flag("HPF_BORDER_GJ_MFMA", s.border_gj_mfma);
    if (const char* v = find("HPF_BORDER_PIVLIM"))
        if (atof(v) > 0.0) s.border_pivlim = atof(v);
    if (const char* v = find("HPF_MESH_BATCH_GB")) {
        s.mesh_batch_gb = atof(v);
        s.mesh_batch_gb_given = true;
    }
    return s;
}

// the process's opt-in to switches from the environment
inline bool env_switches_opted_in() {
    const char* es = getenv("HPF_ENV_SWITCHES");
    return es && atoi(es) != 0;
}

}  // namespace hpf
