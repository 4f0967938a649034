"""Flat-parameter packing: module parameters as views into one contiguous fp32 buffer.

The HIP learner addresses every parameter by offset into a single device buffer (include/mq_learner.h,
MQ_P_*). nn.Module parameters stay ordinary `nn.Parameter`s with the reference's names, so `state_dict()`,
`load_state_dict()`, `parameters()` and the agent.th / mixer.th / opt.th checkpoint files are unchanged
(reference: q_learner.py:131-143, basic_controller.py:91-92).
"""
import torch as th


def pack(modules, flat=None, device=None):
    """Copy the parameters of `modules` (in order) into `flat` (allocated if None) and re-point them at it."""
    params = [p for m in modules for p in m.parameters()]
    total = sum(p.numel() for p in params)
    if flat is None:
        dev = device if device is not None else (params[0].device if params else "cpu")
        flat = th.empty(total, dtype=th.float32, device=dev)
    assert flat.numel() >= total and flat.dtype == th.float32
    o = 0
    with th.no_grad():
        for p in params:
            n = p.numel()
            view = flat[o:o + n].view_as(p)
            view.copy_(p.data)
            p.data = view
            o += n
    return flat, total


def rebind(modules, flat):
    """Re-point parameters at `flat` without copying (after the buffer moved devices)."""
    o = 0
    for m in modules:
        for p in m.parameters():
            n = p.numel()
            p.data = flat[o:o + n].view_as(p)
            o += n
    return o


def state_buffers(optim_name, sq, m):
    """Optimiser-state key -> flat buffer, in torch's key order: Adam's exp_avg in `m` and exp_avg_sq in `sq`, where
    RMSprop's square_avg lives."""
    return {"exp_avg": m, "exp_avg_sq": sq} if optim_name == "adam" else {"square_avg": sq}


def link(params, opt, grad, state):
    """Point every p.grad and optimiser-state tensor of `params` (in order) at its slice of a flat buffer: `grad`, and
    `state`'s key -> buffer (state_buffers). A "step" entry in `state` is ONE tensor shared by every parameter, set in
    its place among the keys; without it each parameter keeps (or gets) a step tensor of its own."""
    o = 0
    for p in params:
        n = p.numel()
        p.grad = grad[o:o + n].view_as(p)
        st = opt.state[p]
        for key, buf in state.items():
            st[key] = buf if key == "step" else buf[o:o + n].view_as(p)
        st.setdefault("step", th.tensor(0.0))
        o += n


def written_by(sd):
    """"adam", "rmsprop" or None: the optimiser whose state_dict `sd` is, by its param_groups' keys."""
    group = (sd.get("param_groups") or [{}])[0]
    return "adam" if "betas" in group else "rmsprop" if "alpha" in group else None


def load_state(opt, sd, params, state, expect=None, what=None, names=str):
    """opt.load_state_dict(sd), then copy the loaded tensors into the flat buffers `state` (key -> buffer):
    load_state_dict replaced the views `link` made, so re-link afterwards. `expect` ("adam" / "rmsprop") switches the
    refusal of a file `what` that the other optimiser wrote on: it would load without complaint (torch checks only the
    group sizes) and leave the moments this learner steps with at zero. Returns the first parameter's step count
    (None: the file holds no steps)."""
    wrote = written_by(sd) if expect is not None else None
    if wrote not in (None, expect):
        raise ValueError("{} was written by {}, but this learner runs optimizer: {}.".format(what, names(wrote),
                                                                                              expect))
    opt.load_state_dict(sd)
    o = 0
    for p in params:
        n = p.numel()
        st = opt.state.get(p, {})
        for key, buf in state.items():
            if key in st:
                buf[o:o + n].copy_(st[key].reshape(-1))
        o += n
    return next((int(float(opt.state[p]["step"])) for p in params if "step" in opt.state.get(p, {})), None)


def state_dict_own_steps(opt):
    """opt.state_dict() with a step tensor per parameter, as torch writes them: the live state may share one counter,
    and a loader that kept it shared would count every parameter's update into it."""
    sd = opt.state_dict()
    sd["state"] = {i: dict(v, step=v["step"].clone()) if "step" in v else v for i, v in sd["state"].items()}
    return sd


def to_current_device(owner, names):
    """Move the tensors `owner.<name>` to the current HIP device, skipping those that are None."""
    dev = th.device("cuda", th.cuda.current_device())
    for name in names:
        t = getattr(owner, name)
        if t is not None:
            setattr(owner, name, t.to(dev))


class FlatModule(th.nn.Module):
    """nn.Module whose parameters live in `self._flat`; device moves keep the flat layout."""

    def _init_flat(self):
        self._flat, _ = pack([self])

    def flat_params(self):
        return self._flat

    def _apply(self, fn, recurse=True):
        flat = getattr(self, "_flat", None)
        if flat is None:
            return super()._apply(fn, recurse)
        new = fn(flat)
        if new is not flat:
            self._flat = new
        rebind([self], self._flat)
        return self

    def __deepcopy__(self, memo):
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k == "_flat":
                continue
            import copy
            setattr(new, k, copy.deepcopy(v, memo))
        new._flat, _ = pack([new], device=self._flat.device)
        return new
