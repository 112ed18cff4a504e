"""The struct-of-arrays batch state, defined once: what DetMADNState, ClassicMADNState and DOGState (detmadn.py,
classic.py, dog.py) share.  A state holds B games as field-major device tensors -- a 2-D field is [rows, B], a 1-D field
[B] -- and the kernels read it through a ctypes struct of the fields' addresses and the batch stride (include/muz.h).

A state class is a dataclass of its tensors, ``rules`` and ``num_players`` (DOG: and ``seed``) that declares

    ROWS     {2-D field: rows as a function of the player count P}
    VECTORS  (1-D fields)
    DTYPES   {field: dtype} where it is not int8
    STRUCT   its ctypes struct (fields of the same names, then ``stride``)

and gets allocation, the struct, gather / scatter of games and clone from here.  A new field is added to the
dataclass, to one of the two declarations and to the struct.
"""
from __future__ import annotations

import torch

from . import lib as _L


def make_rules(defaults: dict, num_players=4, layout=(True, True, True, True), distance=10, starting_player=0, **rules):
    """muz_rules of a game whose env_reset keyword defaults are ``defaults``; an unknown rule is a TypeError."""
    r = dict(defaults)
    unknown = set(rules) - set(r)
    if unknown:
        raise TypeError(f"unknown rule(s): {sorted(unknown)}")
    r.update(rules)
    c = _L.MuzRules()
    c.num_players = int(num_players)
    c.distance = int(distance)
    for i in range(4):
        c.layout[i] = int(bool(layout[i]))
    c.starting_player = int(starting_player)
    for k, v in r.items():
        setattr(c, k, int(bool(v)))
    return c


class SoAState:
    """SoA batch state. Field c of game b is ``field[c, b]``."""

    ROWS, VECTORS, DTYPES, STRUCT, FIELDS = {}, (), {}, None, ()

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        cls.FIELDS = tuple(cls.ROWS) + tuple(cls.VECTORS)

    @classmethod
    def alloc(cls, batch: int, P: int, rules, device, **extra):
        """An uninitialised state of ``batch`` games of ``P`` players."""
        shape = {k: (rows(P), batch) for k, rows in cls.ROWS.items()}
        shape.update((k, (batch,)) for k in cls.VECTORS)
        return cls(**{k: torch.empty(sh, dtype=cls.DTYPES.get(k, torch.int8), device=device)
                      for k, sh in shape.items()}, rules=rules, num_players=P, **extra)

    @property
    def batch(self) -> int:
        return self.current_player.shape[0]

    def soa(self):
        s = self.STRUCT()
        for k in self.FIELDS:
            setattr(s, k, getattr(self, k).data_ptr())
        s.stride = self.batch
        return s

    def pins_bp(self) -> torch.Tensor:
        """pins as [B, P, 4] (the reference's per-game layout)."""
        return self.pins.T.reshape(self.batch, self.num_players, 4)

    def _shallow(self):
        """A second state object over the same tensors and plain attributes (copy.copy costs 3 us more a call)."""
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        return new

    def _games(self, k: str, idx):
        return (slice(None), idx) if k in self.ROWS else idx

    def take(self, idx):
        """The games ``idx`` (an index tensor or a slice) as a state of their own, every field contiguous; ``rules``
        and the other plain attributes are carried over.  An index tensor copies; a slice of a 1-D field is a view."""
        sub = self._shallow()
        for k in self.FIELDS:
            setattr(sub, k, getattr(self, k)[self._games(k, idx)].contiguous())
        return sub

    def put(self, idx, sub):
        """The inverse of ``take``: the games of ``sub`` written over the games ``idx``."""
        for k in self.FIELDS:
            getattr(self, k)[self._games(k, idx)] = getattr(sub, k)

    def clone(self):
        new = self._shallow()
        for k in self.FIELDS:
            setattr(new, k, getattr(self, k).clone())
        return new
