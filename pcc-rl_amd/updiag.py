"""Update diagnostics and the KL guard on the device (include/pcc_policy.h: pcc_policy_act_rows_pop, pcc_update_diag_pop; DESIGN.md
section 23): after an epoch of an update, every member's approximate KL divergence between the rollout's policy and the updated one,
the clip fraction over the whole rollout and the explained variance of the value function; and, with a limit, the per-member
decision to stop updating, taken by the kernel and handed to the optimiser step as a `live` copy of the hyper block -- no copy to the
host, no synchronise.  There is no framework path: the HIP library does the work or the call raises."""
import torch

from .env import _ptr
from .native import call, current_stream, lib

HYPER_COLS = 8   # a row of the population's `hyper` block (include/pcc_policy.h)
DIAG_COLS = 8    # a row of `diag`
DIAG_NAMES = ("count", "approx_kl", "clip_fraction", "explained_variance", "max_log_ratio", "var_ret", "var_resid", "nonfinite")


class UpdateDiagnostics(object):
    """The buffers of the checks of ONE update: mean_new [T][n_envs] float32 (the updated policies' means on the selected rows), diag
    [members][8] float64 (DIAG_NAMES), stop [members] int32 (0, or the epoch at which the member was stopped), hyper_live
    [members][8] float32 (hyper, with lr = 0 for a stopped member) and the kernels' scratch.  Member m owns the columns
    m * n_envs / members ... of every [T][n_envs] row.  row_step: the checks read the rows 0, row_step, 2 row_step, ... only."""

    def __init__(self, n_envs, members=1, device="cuda:0", row_step=1):
        self.n_envs, self.members, self.row_step = int(n_envs), int(members), int(row_step)
        if not 1 <= self.members <= 1024 or self.n_envs < 1 or self.n_envs % self.members != 0:
            raise ValueError("UpdateDiagnostics: %d envs do not divide into %d members (1 .. 1024)" % (self.n_envs, self.members))
        if self.row_step < 1:
            raise ValueError("UpdateDiagnostics: row_step = %r (>= 1)" % (row_step,))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("UpdateDiagnostics runs HIP kernels: it needs a GPU device (device=%r); there is no CPU path" % (device,))
        self.diag = torch.zeros((self.members, DIAG_COLS), dtype=torch.float64, device=self.device)
        self.stop = torch.zeros(self.members, dtype=torch.int32, device=self.device)
        self.hyper_live = torch.zeros((self.members, HYPER_COLS), dtype=torch.float32, device=self.device)
        self.mean_new = None
        self._scratch = None

    def begin(self, hyper):
        """The start of an update: nobody is stopped, hyper_live is hyper.  Two launches, no synchronise."""
        if not (torch.is_tensor(hyper) and hyper.is_cuda and hyper.dtype == torch.float32 and hyper.is_contiguous()
                and tuple(hyper.shape) == (self.members, HYPER_COLS)):
            raise ValueError("UpdateDiagnostics.begin: expected the contiguous float32 hyper block [%d][%d] on the GPU, got %s %s"
                             % (self.members, HYPER_COLS, tuple(getattr(hyper, "shape", ())), getattr(hyper, "dtype", type(hyper))))
        self.stop.zero_()
        self.hyper_live.copy_(hyper)

    def _rows(self, x, what, T):
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() == T * self.n_envs):
            raise ValueError("UpdateDiagnostics.check: expected contiguous float32 %s rows [%d][%d] on the GPU, got %s %s"
                             % (what, T, self.n_envs, tuple(getattr(x, "shape", ())), getattr(x, "dtype", type(x))))
        return x

    def check(self, epoch, obs_b, act_b, logp_b, ret, val_b, flat, param_stride, n_params, arch, hyper, kl_limit=0.0):
        """After epoch `epoch` (1, 2, ...): the updated policies' means on the selected rows of obs_b [T][N][D] (one library call: the
        policy kernel's launches), then the diagnostics and the decision (one library call: two launches).  flat: the parameter
        blocks [members][param_stride] (one member: [>= n_params], param_stride the next multiple of 64); hyper: the [members][8]
        block; kl_limit <= 0: diagnostics only, nobody is stopped.  Nothing synchronises: rows() reads the results."""
        if not (torch.is_tensor(obs_b) and obs_b.is_cuda and obs_b.dtype == torch.float32 and obs_b.is_contiguous() and obs_b.dim() == 3
                and obs_b.shape[1] == self.n_envs):
            raise ValueError("UpdateDiagnostics.check: expected contiguous float32 observation rows [T][%d][D] on the GPU, got %s"
                             % (self.n_envs, tuple(getattr(obs_b, "shape", ()))))
        T, N, D = obs_b.shape
        act_b, logp_b = self._rows(act_b, "action", T), self._rows(logp_b, "log-probability", T)
        ret, val_b = self._rows(ret, "return", T), self._rows(val_b, "value", T)
        need = lib().pcc_update_diag_scratch_doubles(T, self.row_step, N, self.members)
        if need < 0:
            raise ValueError("UpdateDiagnostics.check: a rollout of %d x %d is outside the library's domain" % (T, N))
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.float64, device=self.device)
        if self.mean_new is None or tuple(self.mean_new.shape) != (T, N):
            self.mean_new = torch.zeros((T, N), dtype=torch.float32, device=self.device)
        stream = current_stream(self.device)
        call("pcc_policy_act_rows_pop", _ptr(obs_b), T, self.row_step, N, D, _ptr(flat), int(param_stride), self.members, int(arch[0]),
             int(arch[1]), _ptr(self.mean_new), None, stream)
        call("pcc_update_diag_pop", _ptr(act_b), _ptr(logp_b), _ptr(self.mean_new), _ptr(ret), _ptr(val_b), T, self.row_step, N,
             self.members, _ptr(flat), int(param_stride), (int(n_params) - 1) // 2, _ptr(hyper), float(kl_limit), int(epoch),
             _ptr(self.diag), DIAG_COLS, _ptr(self.stop), _ptr(self.hyper_live), _ptr(self._scratch), stream)

    def rows(self):
        """(diag as `members` lists of 8 numbers, stop as a list) of the last check.  A synchronise: for logging."""
        return self.diag.tolist(), self.stop.tolist()

    def report(self, epochs):
        """The per-member lists a trainer's update() adds to its result, from the last check: approx_kl, clip_fraction,
        explained_variance, max_log_ratio, nonfinite and epochs_run (the epoch at which the member was stopped, or `epochs`)."""
        diag, stop = self.rows()
        out = {name: [r[c] for r in diag] for c, name in enumerate(DIAG_NAMES) if name in
               ("approx_kl", "clip_fraction", "explained_variance", "max_log_ratio")}
        out["nonfinite"] = [int(r[7]) for r in diag]
        out["epochs_run"] = [int(s) if s else int(epochs) for s in stop]
        return out
