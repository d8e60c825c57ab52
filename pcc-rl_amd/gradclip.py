"""Gradient-norm clipping and the non-finite guard beside the fused PPO step (include/pcc_policy.h: pcc_ppo_minibatch_step_clip_pop;
DESIGN.md section 24): the buffers an optimiser step with a limit on the gradient norm needs next to the step's own, and what an
update() reports from them.  The limit itself is column 5 of the population's hyper block.  There is no framework path: the HIP
library does the work or the call raises."""
import torch

HYPER_COLS = 8   # a row of the population's `hyper` block (include/pcc_policy.h)
CLIP_COLS = 8    # a row of `clip`
CLIP_NAMES = ("sumsq", "norm", "coef", "state", "steps", "clipped_steps", "skipped_steps", "max_norm_seen")
STATES = ("applied", "clipped", "skipped", "gradient_only")   # column 3


class GradClip(object):
    """The buffers of the clipped step of `members` learners: grad [members][param_stride] float32 (every member's summed gradient
    of the last step, as the unclipped step's grad_out), hyper_grad [members][8] float32 (the library's work copy of hyper) and clip
    [members][8] float64 (CLIP_NAMES: the last step's sum of squares, norm, coefficient and state, and since begin() the steps
    applied, clipped and skipped and the largest norm seen)."""

    def __init__(self, param_stride, members=1, device="cuda:0"):
        self.param_stride, self.members = int(param_stride), int(members)
        if not 1 <= self.members <= 1024:
            raise ValueError("GradClip: members = %d (1 .. 1024)" % self.members)
        if self.param_stride < 64 or self.param_stride % 64 != 0:
            raise ValueError("GradClip: param_stride = %d (a multiple of 64 floats)" % self.param_stride)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("GradClip runs HIP kernels: it needs a GPU device (device=%r); there is no CPU path" % (device,))
        self.grad = torch.zeros((self.members, self.param_stride), dtype=torch.float32, device=self.device)
        self.hyper_grad = torch.zeros((self.members, HYPER_COLS), dtype=torch.float32, device=self.device)
        self.clip = torch.zeros((self.members, CLIP_COLS), dtype=torch.float64, device=self.device)

    def begin(self):
        """The start of an update: the accumulated columns are zero.  One launch, no synchronise."""
        self.clip[:, 4:].zero_()

    def rows(self):
        """clip as `members` lists of 8 numbers.  A synchronise: for logging."""
        return self.clip.tolist()

    def report(self):
        """The per-member lists a trainer's update() adds to its result: grad_norm (the last step's), max_grad_norm_seen,
        clipped_steps and skipped_steps since begin()."""
        rows = self.rows()
        return {"grad_norm": [r[1] for r in rows], "max_grad_norm_seen": [r[7] for r in rows],
                "clipped_steps": [int(r[5]) for r in rows], "skipped_steps": [int(r[6]) for r in rows]}


def limits(max_grad_norm, members, who):
    """max_grad_norm -- a scalar or one value per member, each finite and >= 0 (0: the guard alone) -- as `members` floats."""
    try:
        vals = [float(max_grad_norm)] * members
    except (TypeError, ValueError):
        vals = [float(x) for x in max_grad_norm]
    if len(vals) != members:
        raise ValueError("%s: max_grad_norm has %d values for %d members" % (who, len(vals), members))
    for x in vals:
        if not (0.0 <= x < float("inf")):
            raise ValueError("%s: max_grad_norm = %r (finite and >= 0; 0: the non-finite guard alone; None: no clipped step)" % (who, x))
    return vals
