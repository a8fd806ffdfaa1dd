"""One flat arena for the trainable variables of a model (train.GRevNetTrainer, train.EncoderTrainer).

A trainer names its variables ONCE, as an ordered list of slots; everything that depends on the order - sizes, the views the
owners read their parameters through, the views a gradient is written through, the per-tensor bounds - comes out of the one
pass over that list in ParamArena.seat.  Pure layout over torch tensors: nothing here needs a device.

A slot is (owner, attribute, *path): the tensor at getattr(owner, attribute)[path[0]][path[1]]..., e.g.
    (mlp, "params", j, 0)            W of layer j  (params is a list of (W, b) tuples)
    (block, "attn_params", "wq")     an entry of an attention block's dict
    (norm, "gamma")                  a plain attribute
The owner is the object a set_params call re-binds, so that `read` sees the re-binding."""
import torch


def read(slot):
    t = getattr(slot[0], slot[1])
    for i in slot[2:]:
        t = t[i]
    return t


def _replaced(box, path, tensor):
    if not path:
        return tensor
    i, new = path[0], _replaced(box[path[0]], path[1:], tensor)
    if isinstance(box, tuple):
        return box[:i] + (new,) + box[i + 1:]
    box[i] = new
    return box


def write(slot, tensor):
    setattr(slot[0], slot[1], _replaced(getattr(slot[0], slot[1]), slot[2:], tensor))


class ParamArena:
    """theta, grad and Adam's m, v: four flat fp32 vectors of one layout.  After seat(), `views[i]` / `grad_views[i]` are slot
    i's windows of theta / grad (in the tensor's own shape), the owners hold the theta views, `bounds` are the tensors' start
    offsets plus the end of the last (`offsets`: the same as int64 on the device, what a per-tensor reduction reads) and
    `tail` / `grad_tail` are the `trailing` free entries after the last tensor.  `epoch` is the caller's: the value of its
    mutation counter when it last knew the arena seated (is_seated)."""

    def __init__(self):
        self.theta = self.grad = self.m = self.v = self.offsets = self.tail = self.grad_tail = None
        self.slots, self.views, self.grad_views, self.bounds = [], [], [], [0]
        self.epoch = None

    def is_seated(self, device, epoch):
        """Do the owners still read their parameters through this arena, on `device`?  One integer compare while `epoch` is
        the one recorded; else one identity check per variable (no device work, nothing allocated)."""
        if self.theta is None or self.theta.device != torch.device(device):
            return False
        if self.epoch != epoch:
            if not all(read(s) is v for s, v in zip(self.slots, self.views)):
                return False
            self.epoch = epoch
        return True

    def seat(self, slots, device, trailing=0):
        """Lay the slots' current tensors out in order, copy their values in and put the theta views back into the owners.
        grad is zeroed; m and v are kept when the total size and the device are what they were, else zeroed; the trailing
        entries of theta are the caller's to fill.  The caller then tells the owners' caches (version counters) and sets
        `epoch`."""
        tensors = [read(s) for s in slots]
        bounds = [0]
        for t in tensors:
            bounds.append(bounds[-1] + t.numel())
        total = bounds[-1] + int(trailing)
        theta = torch.empty(total, dtype=torch.float32, device=device)
        grad = torch.zeros_like(theta)
        cut = lambda flat: [flat[a:b].view(t.shape) for a, b, t in zip(bounds, bounds[1:], tensors)]
        views, grad_views = cut(theta), cut(grad)
        for s, view, t in zip(slots, views, tensors):
            view.copy_(t)
            write(s, view)
        if self.m is None or self.m.numel() != total or self.m.device != theta.device:
            self.m, self.v = torch.zeros_like(theta), torch.zeros_like(theta)
        self.theta, self.grad, self.tail, self.grad_tail = theta, grad, theta[bounds[-1]:], grad[bounds[-1]:]
        self.slots, self.views, self.grad_views, self.bounds = list(slots), views, grad_views, bounds
        self.offsets = torch.tensor(bounds, dtype=torch.int64, device=device)
        self.epoch = None
        return self
