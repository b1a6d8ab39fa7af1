"""Derived forms of module weights (fp16 NHWC copies, MFMA fragment images, merged or padded weights, cast biases),
cached per owner and rebuilt exactly when one of the tensors they were derived from changes."""
import weakref

import torch


def tensors_key(tensors):
    """What identifies the present content of `tensors`: each one's own storage address and version counter (every
    in-place torch op, load_state_dict and the foreach optimisers advance it), its device and dtype, in order.  Read
    from the tensors as they are NOW: a rebound `.data`, a replaced nn.Parameter and a `.to()` all change it."""
    return tuple((t.data_ptr(), t._version, t.device, t.dtype) for t in tensors)


class WeightPacks:
    """slot -> (key, value).  A per-module pack uses the slot (weakref.ref(module), kind), see conv_pack: the module is
    not kept alive, and the entries of a module that is gone leave at the next rebuild.  A copied or pickled owner
    (deepcopy, mp.spawn) gets an empty cache and re-derives its packs."""

    def __init__(self, entries=None):
        self._entries = {} if entries is None else entries

    def get(self, slot, tensors, build):
        """the value `build()` returned for the current tensors_key(tensors)"""
        key = tensors_key(tensors)
        hit = self._entries.get(slot)
        if hit is None or hit[0] != key:
            for s in [s for s in self._entries if isinstance(s, tuple)
                      and any(isinstance(r, weakref.ref) and r() is None for r in s)]:
                del self._entries[s]
            hit = self._entries[slot] = (key, build())
        return hit[1]

    def __deepcopy__(self, memo):
        return WeightPacks()

    def __reduce__(self):
        return (WeightPacks, ())


def conv_pack(cache, conv, kind, pack, bias_dtype=torch.float32):
    """(pack(conv.weight), the bias as `bias_dtype`) of a convolution: one entry of `cache` per module and `kind`"""
    cache = cache if isinstance(cache, WeightPacks) else WeightPacks(cache)      # a caller's `{}` serves as the store
    return cache.get((weakref.ref(conv), kind), (conv.weight, conv.bias),
                     lambda: (pack(conv.weight), conv.bias.detach().to(bias_dtype).contiguous()))
