// TEST INFRASTRUCTURE: the build-switch parser of csrc/hpf_switches.hpp on the host (tests/test_switches_host.py): defaults, token form,
// precedence of the option string over the environment, the environment only on opt-in, presence-only switches, HPF_TREE_DUMP from the
// environment only.  Prints "switches clean" when every check holds.
#include <stdio.h>
#include <stdlib.h>

#include "hpf_switches.hpp"
using namespace hpf;

static int fails = 0;
#define CHECK(c)                                                 \
    do {                                                         \
        if (!(c)) {                                              \
            printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c);  \
            ++fails;                                             \
        }                                                        \
    } while (0)

int main() {
    const char* names[] = {"HPF_LAZY", "HPF_COMPRESS", "HPF_TREE_INFO", "HPF_TREE_DUMP", "HPF_MESH_BATCH_GB", "HPF_SLEAF"};
    for (const char* n : names) unsetenv(n);

    // defaults
    const Switches d = parse_switches(nullptr, false);
    CHECK(!d.tree_info && !d.border_info && !d.queue_info && d.tree_dump.empty() && d.debug_ablate == 0);
    CHECK(d.gj_mode == 1 && d.n_groups == 4 && d.leafbatch && d.fuse_levels && d.fuse_back && d.fuse_back_max == 32 && d.border_slot_cap == 1024);
    CHECK(d.lintree && d.linbundle && d.chainbundle && d.sleaf == 2 && d.slback && d.sllazy && d.slnest && d.lazy == 2 && d.compress);
    CHECK(d.mesh_sel && d.border_gj == 96 && d.border_gj_mfma && d.border_pivlim == 1e3 && d.mesh_batch_gb == 48.0 && !d.mesh_batch_gb_given);

    // first occurrence wins; values through atoi / atof ("HPF_LAZY=" is 0)
    CHECK(parse_switches("HPF_LAZY=1 HPF_LAZY=0", false).lazy == 1);
    CHECK(parse_switches("HPF_LAZY=", false).lazy == 0);
    CHECK(parse_switches("HPF_GROUPS=0", false).n_groups == 1 && parse_switches("HPF_GROUPS=99", false).n_groups == 8);
    CHECK(parse_switches("HPF_GJ_MODE=7", false).gj_mode == 1 && parse_switches("HPF_GJ_MODE=0", false).gj_mode == 0);
    CHECK(parse_switches("HPF_BORDER_PIVLIM=-1", false).border_pivlim == 1e3 && parse_switches("HPF_BORDER_PIVLIM=2.5", false).border_pivlim == 2.5);

    // separators ' ', ',' and ';'; a name only at the start of a token; unknown names ignored
    const Switches sep = parse_switches("HPF_SLEAF=0,HPF_LAZY=1;HPF_COMPRESS=0 HPF_FOO=1", false);
    CHECK(sep.sleaf == 0 && sep.lazy == 1 && !sep.compress);
    CHECK(parse_switches("XHPF_LAZY=0", false).lazy == 2);

    // a name that is the prefix of another
    const Switches pre = parse_switches("HPF_BORDER_GJ_MFMA=0", false);
    CHECK(pre.border_gj == 96 && !pre.border_gj_mfma);
    const Switches pre2 = parse_switches("HPF_BORDER_GJ_MFMA=1 HPF_BORDER_GJ=5", false);
    CHECK(pre2.border_gj == 5 && pre2.border_gj_mfma);
    CHECK(parse_switches("HPF_FUSEBACK_MAX=8", false).fuse_back && parse_switches("HPF_FUSEBACK_MAX=8", false).fuse_back_max == 8);

    // presence-only switches
    CHECK(parse_switches("HPF_TREE_INFO=0", false).tree_info);
    CHECK(parse_switches("HPF_QUEUE_INFO=", false).queue_info && parse_switches("HPF_BORDER_INFO=0", false).border_info);
    const Switches gb = parse_switches("HPF_MESH_BATCH_GB=2", false);
    CHECK(gb.mesh_batch_gb_given && gb.mesh_batch_gb == 2.0);

    // the environment: only on opt-in, and only for names the string lacks
    setenv("HPF_LAZY", "0", 1);
    setenv("HPF_COMPRESS", "0", 1);
    setenv("HPF_TREE_INFO", "", 1);
    setenv("HPF_MESH_BATCH_GB", "0", 1);
    const Switches off = parse_switches(nullptr, false);
    CHECK(off.lazy == 2 && off.compress && !off.tree_info && !off.mesh_batch_gb_given);
    const Switches on = parse_switches(nullptr, true);
    CHECK(on.lazy == 0 && !on.compress && on.tree_info && on.mesh_batch_gb_given && on.mesh_batch_gb == 0.0);
    const Switches both = parse_switches("HPF_LAZY=1", true);
    CHECK(both.lazy == 1 && !both.compress);

    // HPF_TREE_DUMP: environment only (on opt-in); in an option string it is ignored and the switches after it still apply
    const Switches dump = parse_switches("HPF_TREE_DUMP=/x HPF_SLEAF=0", false);
    CHECK(dump.tree_dump.empty() && dump.sleaf == 0);
    setenv("HPF_TREE_DUMP", "/tmp/plan.txt", 1);
    CHECK(parse_switches(nullptr, false).tree_dump.empty());
    CHECK(parse_switches("HPF_TREE_DUMP=/x", true).tree_dump == "/tmp/plan.txt");

    if (fails) return 1;
    printf("switches clean\n");
    return 0;
}
