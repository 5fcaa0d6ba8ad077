"""The call-order rules of include/hpf.h as a table: for every call of a batch's life the code it must return (HPF_OK, HPF_E_ARG, HPF_E_STATE)
and hpf_num_scenarios afterwards.  Written from the header's sentences, not from csrc/hpf_lib.hip; tests/test_gpu_handle_history.py walks a
handle at random and compares.  Test infrastructure only.  Argument ranges that do not depend on the state come first, then the state, then the
arguments measured against the batch (hpf.h at hpf_set_loads); a call refused by such a host check changes nothing but a refused queue registration."""
OK, E_ARG, E_STATE = 0, -1, -2
RANGES = {"keep_previous_state": None, "auto_repivot": None, "block_pivoting": None, "step_residual_check": (0, 1), "rectangular_update": (0, 1),
          "queue_chunk": (1, 16), "scenario_groups": (1, 8), "pivot_growth_limit_log10": (0, 300)}


class Contract:
    def __init__(self, s_max):
        self.s_max, self.S, self.pending = s_max, 0, 0        # pending: scenarios of a registration of hpf_queue_sources
        self.loads = self.state = self.mm = self.solved = self.records = self.src = self.start = self.prev = False
        self.opt = {name: 0 for name in RANGES}                # (keep_previous_state, step_residual_check and block_pivoting decide codes)
        self.open = {"distortion": False, "branch_stats": False, "waveform_stats": False}

    def num_scenarios(self):
        return self.S if self.loads or self.state else 0

    def _batch(self, S, loads, state, src):                   # a new batch or state ends the mismatch, the kept state, "solve was last", the records
        self.S, self.loads, self.state, self.src = S, loads, state, src
        self.mm = self.prev = self.solved = self.records = False
        return OK

    def set_loads(self, k):                                   # a state of the same size is kept, sources are dropped
        return E_ARG if k > self.s_max else self._batch(k, True, self.state and k == self.S, False)

    def set_state(self, k, apply=False):
        if k > self.s_max:
            return E_ARG
        if apply and not self.start:
            return E_STATE
        return E_ARG if self.loads and k != self.S else self._batch(k, self.loads, True, self.src)

    def set_sources(self, rows):
        if not self.loads or rows != self.S:
            return E_ARG if self.loads else E_STATE
        self.src, self.mm, self.solved = True, False, False
        return OK

    def clear_sources(self):                                  # a batch without sources is not touched; a pending registration goes too
        self.mm, self.solved = self.mm and not self.src, self.solved and not self.src
        self.src, self.pending = False, 0
        return OK

    def queue_sources(self, k):
        self.pending = k
        return OK

    def solve_queue(self, k):                                 # a registration for another sweep: refused and dropped; else no batch afterwards
        pending, self.pending = self.pending, 0
        return E_ARG if pending not in (0, k) else self._batch(0, False, False, False)

    def start_state(self, what):                              # set / capture / get / clear
        if (what == "capture" and not self.state) or (what == "get" and not self.start):
            return E_STATE
        self.start = self.start if what == "get" else what != "clear"
        return OK

    def run(self, what):                                      # mismatch / iterate / fund_pf / solve
        if not (self.loads and self.state) or (what == "iterate" and not self.mm):
            return E_STATE
        if what == "solve":                                   # (prev: for the scenarios that took a step -- the caller knows from n_iter)
            self.records, self.prev = True, bool(self.opt["keep_previous_state"])
        self.mm = what in ("mismatch", "iterate")             # (iterate was only accepted with a valid one)
        self.solved = what == "solve" or (what == "mismatch" and self.solved)
        return OK

    def read(self, what):
        need = {"get_stats": self.records, "get_sources": self.src, "step_residuals": self.opt["step_residual_check"] and self.state,
                "jacobian_last": self.opt["keep_previous_state"] and self.prev, "branch_flows": self.state, "waveform": self.state}[what]
        return OK if need else E_STATE

    def accum(self, which, what):                             # begin / add / get / end
        if what in ("begin", "end"):
            self.open[which] = what == "begin"
            return OK
        return OK if self.open[which] and (what == "get" or self.solved) else E_STATE

    def set_option(self, name, value):
        if name not in RANGES or (RANGES[name] and not RANGES[name][0] <= value <= RANGES[name][1]):
            return E_ARG
        if name == "block_pivoting" and bool(value) != bool(self.opt[name]):
            self.mm = False                                   # the two modes keep the mismatch in different layouts
        self.opt[name] = value
        return OK
