"""The engine's rule switches: which planner, scheduler and executor rules a plan is built with (host logic, no GPU needed).

One `RuleSet` is made when a plan is built (planner.build_plan), the whole plan is built under it and `Plan.rules` keeps it:
the executor binds every batch size of that plan under the same set.  The defaults are the product; the switches exist for A/B
measurements.  `RuleSet.from_env` reads them from the environment -- field `x` is the variable DEEPHAR_X -- and is what
build_plan uses when it is given no rules (`Model.rules = None`)."""
import dataclasses
import os


@dataclasses.dataclass(frozen=True)
class RuleSet:
    # ---- planner (engine/planner.py) ----
    split_adds: bool = True         # R9 + second-add rule; off: wide adds stay element-wise launches (re-orders fp32 sums)
    up_commute: bool = True         # R11 up-scaling unit at half resolution; off: UpSampling2D is written out (re-orders two adds)
    resample_on_load: bool = True   # R12 skinny-conv kernel pools / up-samples while loading; off: the resampled tensor is written
    concat_shared: bool = True      # R4b a tensor read by a concatenation and by view readers lives inside it; off: a copy launch
    merge_heads: bool = True        # R10 sibling convolutions filling neighbouring slabs are one launch; off: one launch each
    merge_kxk: bool = True          # R10b R10 also for K x K siblings of different extents; off: 1x1 siblings only
    merge_siblings: bool = True     # R10c sibling 1x1 convolutions with outputs of their own share a joint buffer; off: apart
    merge_pools: bool = True        # R13 two poolings into one concatenation are one launch; off: two
    pool_segments: bool = True      # R14 skinny-conv kernel reads concatenate([pool(x), x2]) in place; off: the pooling is written
    res2_down: bool = True          # R3 up-sampled second residual read at half resolution; off: conv -> up-sample -> add forms
    fuse_pool: bool = True          # R7 MaxPooling2D((2, 2)) in the epilogue of the producing convolution; off: a pooling launch
    fuse_pool_small: bool = True    # R7 also behind 16- and 8-column outputs; off: 32 columns only
    fold_pose_mul: bool = True      # multiply([pose, confidence]) inside the soft-argmax launch; off: a multiply launch
    # ---- executor (engine/executor.py) ----
    halo_conv: bool = True          # halo-resident K x K kernel where the library takes the layer; off: the general kernel
    group_launches: bool = True     # (1x1 shortcut conv, depthwise conv) pairs are one launch at small batches; off: two
    pair_convs: bool = True         # two independent skinny convolutions are one launch at small batches; off: two
    # ---- scheduler (engine/schedule.py: assign_streams_tail) ----
    tail_floor_us: float = 30.0     # per-launch cost of the 'tail' policy's makespan model (calibration sweeps)
    tail_shift: int = 0             # moves the start of the 'tail' policy's suffix by this many steps (A/B aid)

    @classmethod
    def from_env(cls, environ=os.environ):
        """A boolean rule is on unless its variable is the string '0'; the two numbers are parsed as float / int."""
        kw = {}
        for f in dataclasses.fields(cls):
            raw = environ.get('DEEPHAR_' + f.name.upper())
            if raw is not None:
                kw[f.name] = raw != '0' if f.type is bool else f.type(raw)
        return cls(**kw)
