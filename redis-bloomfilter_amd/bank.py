"""``BloomfilterBank`` — many ``Redis::Bloomfilter`` key names of one size and error rate on
one device allocation (a ``bf_bank``, include/bfhip.h).

In the reference ``key_name`` names a filter (lib/redis/bloomfilter.rb:14, ruby.rb:33-35, 59)
and an application keeps one per tenant, per day or per feed.  A bank fixes the list of key
names at construction (``key_names[i]`` is filter ``i``), sizes every filter with
``Bloomfilter.optimal_m`` / ``optimal_k`` (bloomfilter.rb:25-28) and takes a mixed batch of
``(key name, key)`` pairs in one launch.  ``first_seen_many`` is first-seen dedup over such a
batch: insert, and say per pair whether it was new, exactly as if the pairs had gone in one by
one (bf_bank_insert_many_seq).  ``which`` / ``include_across`` ask the question only a
bank can answer in one launch: which of the key names have seen this key.  ``merge`` / ``rollup``
/ ``union_size`` / ``intersection_size`` / ``overlap`` combine key names with each other on the
device (bf_bank_fold, bf_bank_overlap).

Redis sync follows ``drivers/hip.py``'s contract, per key name:

* attach (``redis=``): every key name that exists is imported (a filter written by the ruby
  driver is readable here) and its PTTL mirrored;
* ``sync='write_through'`` (default): after an insert each key name whose string CHANGED is
  written back, its trimmed string with ``SETRANGE name 0`` (keeps the TTL; under OR a string
  only grows, so the key becomes exactly the string the ruby driver's SETBITs build), followed
  by EXPIRE when ``expire`` is given — ruby.rb:61-62, per key name;
* ``sync='write_through_bits'``: the same, but an insert asks the device WHICH bits it flipped
  (bf_bank_insert_many_changes) and a key name that changed by only a few bits gets exactly the
  SETBITs the ruby driver would have sent that changed something (ruby.rb:58-60) instead of its
  whole string: ``bank[name].insert(key)`` then sends at most k SETBITs, not ceil(m / 8) bytes.
  A key name with more flipped bits than k and than ``ceil(m / 8) / SETBIT_BYTES`` (the hip
  driver's cost model) is written whole as above.  A SETBIT keeps the TTL and grows the string as the
  reference's does, so Redis ends byte for byte where the default mode leaves it;
* ``sync='manual'``: Redis is touched only by ``flush`` / ``reload`` / ``clear``;
* TTL: when a key name's mirrored deadline passes, that one filter is cleared, as the Redis key
  would have vanished.
"""
from __future__ import annotations

import time
from typing import Dict, Iterable, List, Optional, Sequence, Set

import numpy as np

from . import fakeredis
from . import keys as _keys
from ._lib import ArgumentError, BF_IMPORT_REPLACE, FilterBank, estimate_count
from .bloomfilter import Bloomfilter
from .drivers.hip import Hip


class BankFilter:
    """``bank[name]``: the reference's ``insert`` / ``include`` / ``clear`` for one key name."""

    def __init__(self, bank: "BloomfilterBank", name: str):
        self.bank, self.key_name = bank, name

    def insert(self, data, expire=None):
        return self.bank.insert(self.key_name, data, expire)

    def first_seen(self, key, expire=None) -> bool:
        return self.bank.first_seen(self.key_name, key, expire)

    def include(self, key) -> bool:
        return self.bank.include(self.key_name, key)

    __contains__ = include

    def clear(self):
        return self.bank.clear(self.key_name)


class BloomfilterBank:
    SYNC_MODES = ("write_through", "manual", "write_through_bits")

    def __init__(self, size=None, error_rate=None, key_names: Optional[Sequence] = None, redis=None,
                 sync: str = "write_through", default_expire=None, device: int = -1, clock=time.monotonic):
        # bloomfilter.rb:21
        if error_rate is None or size is None:
            raise ArgumentError("options[:size] && options[:error_rate] cannot be nil")
        names = [str(n) for n in (key_names or [])]
        if not names:
            raise ArgumentError("key_names must list at least one key name")
        if len(set(names)) != len(names):
            dup = sorted(n for n in set(names) if names.count(n) > 1)
            raise ArgumentError("key_names repeats %r" % dup[0])
        if sync not in self.SYNC_MODES:
            raise ArgumentError("sync must be one of %s" % (self.SYNC_MODES,))
        self.options = {"size": size, "error_rate": error_rate, "default_expire": default_expire,
                        "bits": Bloomfilter.optimal_m(size, error_rate)}
        self.options["hashes"] = Bloomfilter.optimal_k(size, self.options["bits"])   # bloomfilter.rb:25-28
        if self.options["bits"] <= 0:
            raise ArgumentError("filter size in bits must be positive (got %r)" % (self.options["bits"],))
        self.key_names: List[str] = names
        self.ids: Dict[str, int] = {n: i for i, n in enumerate(names)}
        self.sync_mode = sync
        self._clock = clock
        self.bank = FilterBank(self.options["bits"], self.options["hashes"], len(names), device=device)
        self._deadline: Dict[int, float] = {}
        self._dirty: Set[int] = set()    # manual sync: filters changed since the last flush
        self._replaced: Set[int] = set()   # ... of those, a rollup replaced: flush DELetes them first
        self.redis = redis if redis is not None else fakeredis.current()   # bloomfilter.rb:30
        self.reload()

    # -- helpers
    def _id(self, name) -> int:
        try:
            return self.ids[str(name)]
        except KeyError:
            raise ArgumentError("unknown key name %r" % (name,)) from None

    def _expire(self, expire):
        """``expire || @options[:default_expire]`` (bloomfilter.rb:62)."""
        return self.options["default_expire"] if expire is None or expire is False else expire

    def _batch(self, names, keys):
        names, keys = list(names), list(keys)
        if len(names) != len(keys):
            raise ArgumentError("%d key names for %d keys" % (len(names), len(keys)))
        ids = np.array([self._id(n) for n in names], np.uint32)
        buf, offs = _keys.pack(keys)
        return ids, buf, offs

    def _expired(self) -> None:
        """Clear every filter whose mirrored deadline has passed (and DEL it, write-through)."""
        if not self._deadline:
            return
        now = self._clock()
        due = [i for i, t in self._deadline.items() if now >= t]
        if not due:
            return
        self.bank.clear(np.array(due, np.uint32))
        for i in due:
            del self._deadline[i]
            self._dirty.discard(i)
            self._replaced.discard(i)
            if self.redis is not None and self.sync_mode != "manual":
                self.redis.delete(self.key_names[i])

    def _write(self, ids: Sequence[int]) -> int:
        """SETRANGE name 0 <trimmed string> for every listed filter; returns the bytes sent."""
        ids = sorted(ids)
        if not ids or self.redis is None:
            return 0
        sent = 0
        for i, s in zip(ids, self.bank.export_redis(np.array(ids, np.uint32))):
            if s:
                self.redis.setrange(self.key_names[i], 0, s)
                sent += len(s)
        return sent

    # -- ruby.rb:15-17 / 57-63, per key name
    def insert_many(self, names: Iterable, keys: Iterable, expire=None) -> Set[str]:
        """Key j goes into the filter named names[j].  Returns the set of key names whose string
        changed (the reference's ``!found`` per key name)."""
        self._expired()
        ids, buf, offs = self._batch(names, keys)
        if self.sync_mode == "write_through_bits":
            _, lids, lbits = self.bank.insert_many_changes(buf, offs, ids)
            return self._inserted(lids, None, expire, lbits)
        flipped = self.bank.insert_many(buf, offs, ids)
        return self._inserted(ids, flipped, expire)

    # One SETBIT costs the server about as much as SETRANGEing this many bytes: the hip driver's
    # cost model and its one constant (drivers/hip.py).
    SETBIT_BYTES = Hip.SETBIT_BYTES

    def _write_bits(self, lids: np.ndarray, lbits: np.ndarray) -> None:
        """``write_through_bits``: per changed key name, the flipped bits as SETBIT name o 1
        (ruby.rb:58-60; pipelined when the client can) while they cost less than the string
        ``_write`` would send, else that string.  ceil(m / 8) bounds the string, so no filter is
        exported just to decide.  As in the hip driver, what a per-key call can flip (k bits, no
        more than the reference's own k SETBITs for that key) is always replayed."""
        order = np.argsort(lids, kind="stable")
        lids, lbits = lids[order], lbits[order]
        names, starts = np.unique(lids, return_index=True)
        ends = list(starts[1:]) + [len(lids)]
        string_bytes = -(-self.options["bits"] // 8)
        k = self.options["hashes"]
        whole, replay = [], []
        for i, s, e in zip(names.tolist(), starts.tolist(), ends):
            if e - s <= k or (e - s) * self.SETBIT_BYTES <= string_bytes:
                replay.append((self.key_names[i], lbits[s:e].tolist()))
            else:
                whole.append(i)
        if replay:
            pipe = getattr(self.redis, "pipeline", None)
            r = pipe(transaction=False) if pipe is not None else self.redis
            for name, offsets in replay:
                for o in offsets:
                    r.setbit(name, o, 1)
            if pipe is not None:
                r.execute()
        self._write(whole)

    def _inserted(self, ids: np.ndarray, new: Optional[np.ndarray], expire, bits: Optional[np.ndarray] = None) -> Set[str]:
        """The Redis side of an insert, per key name whose string changed (``ids[new != 0]``; with
        ``bits``, the list of bf_bank_insert_many_changes: its distinct ids): write-through
        SETRANGE / SETBITs or dirty marking, EXPIRE and deadline arming (ruby.rb:61-62).
        Returns those key names."""
        changed = sorted(set((ids if bits is not None else ids[new != 0]).tolist()))
        expire = self._expire(expire)
        armed = expire is not None and expire is not False   # ruby.rb:62: 0 counts
        write = self.redis is not None and self.sync_mode != "manual"
        if write and bits is not None:
            self._write_bits(ids, bits)
        elif write:
            self._write(changed)
        else:
            self._dirty.update(changed)
        if armed:
            t0 = self._clock()
            for i in changed:
                self._deadline[i] = t0 + float(expire)
                if write:
                    self.redis.expire(self.key_names[i], expire)
        return {self.key_names[i] for i in changed}

    def insert(self, name, key, expire=None) -> bool:
        return bool(self.insert_many([name], [key], expire))

    # -- first-seen dedup: benchmark/bf_10_000.rb:34-43's include? then insert, per key name
    def first_seen_many(self, names: Iterable, keys: Iterable, expire=None) -> np.ndarray:
        """Insert the batch and answer, per pair, "had I seen this before?" negated: [j] is True iff
        ``(names[j], keys[j])`` was not in its filter before its own insert, the pairs taken one
        at a time in batch order (so a pair repeated in the batch is True at its first place only).
        Towards Redis it behaves like ``insert_many``."""
        self._expired()
        ids, buf, offs = self._batch(names, keys)
        if self.sync_mode == "write_through_bits":
            new, lids, lbits = self.bank.insert_many_changes(buf, offs, ids, seq=True)
            self._inserted(lids, None, expire, lbits)
        else:
            new = self.bank.insert_many_seq(buf, offs, ids)
            self._inserted(ids, new, expire)
        return new.astype(bool)

    def first_seen(self, name, key, expire=None) -> bool:
        return bool(self.first_seen_many([name], [key], expire)[0])

    # -- ruby.rb:20-30
    def include_many(self, names: Iterable, keys: Iterable) -> np.ndarray:
        self._expired()
        ids, buf, offs = self._batch(names, keys)
        return self.bank.include_many(buf, offs, ids).astype(bool)

    def include(self, name, key) -> bool:
        return bool(self.include_many([name], [key])[0])

    # -- ruby.rb:20-30 of one key in many key names: the key is hashed once (bf_bank_include_across)
    def include_across(self, keys: Iterable, names: Optional[Iterable] = None) -> np.ndarray:
        """A bool array of shape (len(keys), len(names)): [j, i] = ``include(names[i], keys[j])``.
        ``names`` defaults to every key name, in ``key_names`` order.  A read: Redis is not touched."""
        self._expired()
        ids = None if names is None else np.array([self._id(n) for n in names], np.uint32)
        buf, offs = _keys.pack(list(keys))
        return self.bank.include_across(buf, offs, ids)

    def which(self, key, names: Optional[Iterable] = None) -> List[str]:
        """The key names whose filter contains ``key``, in ``names`` order (default: ``key_names``)."""
        listed = self.key_names if names is None else [str(n) for n in names]
        hits = self.include_across([key], None if names is None else listed)[0]
        return [n for n, hit in zip(listed, hits) if hit]

    # -- ruby.rb:33-35
    def clear(self, name=None) -> None:
        """DEL one key name's filter, or every one (``name=None``)."""
        ids = list(range(len(self.key_names))) if name is None else [self._id(name)]
        self.bank.clear(None if name is None else np.array(ids, np.uint32))
        for i in ids:
            self._deadline.pop(i, None)
            self._dirty.discard(i)
            self._replaced.discard(i)
        if self.redis is not None:
            self.redis.delete(*[self.key_names[i] for i in ids])

    def __getitem__(self, name) -> BankFilter:
        self._id(name)
        return BankFilter(self, str(name))

    # -- statistics
    def count_bits(self) -> np.ndarray:
        """BITCOUNT of every key name, in ``key_names`` order, counted on the device."""
        self._expired()
        return self.bank.bitcount()

    def estimated_sizes(self) -> np.ndarray:
        """About how many distinct keys each filter holds (``estimate_count`` of its bit count)."""
        m, k = self.options["bits"], self.options["hashes"]
        return np.array([estimate_count(m, k, int(x)) for x in self.count_bits()], np.float64)

    # -- key names combined with each other (bf_bank_fold / bf_bank_overlap)
    def _arm(self, i: int, expire, write: bool) -> None:
        """``expire || default_expire`` for filter i, as ``insert_many`` arms a changed key name."""
        expire = self._expire(expire)
        if expire is not None and expire is not False:   # ruby.rb:62: 0 counts
            self._deadline[i] = self._clock() + float(expire)
            if write:
                self.redis.expire(self.key_names[i], expire)

    def merge(self, dst, sources: Iterable, expire=None) -> bool:
        """``dst |= OR(sources)`` on the device (BITOP OR dst dst sources...); True iff dst's string
        changed.  It is then written back (write-through; an OR only grows the string, so SETRANGE
        dst 0 is right) or marked for ``flush``, and ``expire`` armed as by an insert that set a bit."""
        self._expired()
        d = self._id(dst)
        changed = bool(self.bank.fold("or", [[d] + [self._id(n) for n in sources]], [d])[0][0])
        if changed:
            write = self.redis is not None and self.sync_mode != "manual"
            if write:
                self._write([d])
            else:
                self._dirty.add(d)
            self._arm(d, expire, write)
        return changed

    def rollup(self, dst, sources: Iterable, expire=None) -> bool:
        """``dst = OR(sources)``, replacing it ("last 7 days" from seven daily key names); True iff
        dst's string changed.  The string may shrink and SETRANGE never shrinks a key, so the key is
        DELeted and written anew; its TTL goes with the DEL, as in ``clear``, and is armed again
        when the result is non-empty."""
        self._expired()
        d = self._id(dst)
        srcs = [self._id(n) for n in sources]
        if not srcs:
            raise ArgumentError("rollup needs at least one source key name")
        changed, set_bits = self.bank.fold("or", [srcs], [d])
        if changed[0]:
            write = self.redis is not None and self.sync_mode != "manual"
            self._deadline.pop(d, None)
            if write:
                self.redis.delete(self.key_names[d])
                self._write([d])
            else:
                self._dirty.add(d)
                self._replaced.add(d)
            if int(set_bits[0]):
                self._arm(d, expire, write)
        return bool(changed[0])

    def union_size(self, names: Iterable) -> float:
        """Estimated distinct keys of the listed key names together (``estimate_count`` of a
        count-only OR); nothing is modified, Redis is not touched."""
        self._expired()
        _, set_bits = self.bank.fold("or", [[self._id(n) for n in names]])
        return estimate_count(self.options["bits"], self.options["hashes"], int(set_bits[0]))

    def intersection_size(self, a, b) -> float:
        """Estimated keys two key names share, by inclusion-exclusion n(A) + n(B) - n(A or B)."""
        self._expired()
        ia, ib = self._id(a), self._id(b)
        _, bits = self.bank.fold("or", [[ia], [ib], [ia, ib]])
        na, nb, nu = (estimate_count(self.options["bits"], self.options["hashes"], int(x)) for x in bits)
        return na + nb - nu

    def overlap(self, names_a: Optional[Iterable] = None, names_b: Optional[Iterable] = None) -> np.ndarray:
        """uint64 [i, j] = BITCOUNT(names_a[i] AND names_b[j]); ``names_a`` defaults to every key
        name, ``names_b`` to ``names_a``.  A read: Redis is not touched."""
        self._expired()
        rows = None if names_a is None else np.array([self._id(n) for n in names_a], np.uint32)
        cols = None if names_b is None else np.array([self._id(n) for n in names_b], np.uint32)
        return self.bank.overlap(rows, cols)

    # -- Redis sync
    def flush(self, full: bool = False) -> int:
        """Write the filters that changed since the last flush (``full``: every non-empty one).  A
        filter a ``rollup`` replaced is DELeted first: its string may have shrunk."""
        self._expired()
        ids = range(len(self.key_names)) if full else self._dirty
        if self.redis is not None and self._replaced:
            self.redis.delete(*[self.key_names[i] for i in sorted(self._replaced)])
        sent = self._write(list(ids))
        if self.redis is not None:
            self._dirty.clear()
            self._replaced.clear()
        return sent

    def reload(self, names: Optional[Iterable] = None) -> None:
        """Replace the listed filters (default: all) with their Redis keys' current values."""
        if self.redis is None:
            return
        ids = list(range(len(self.key_names))) if names is None else [self._id(n) for n in names]
        have, strings, gone = [], [], []
        for i in ids:
            t0 = self._clock()
            data = self.redis.get(self.key_names[i])
            self._deadline.pop(i, None)
            self._dirty.discard(i)
            self._replaced.discard(i)
            if data is None:
                gone.append(i)
                continue
            have.append(i)
            strings.append(bytes(data))
            ttl = self.redis.pttl(self.key_names[i]) if hasattr(self.redis, "pttl") else -1
            if ttl is not None and ttl > 0:
                self._deadline[i] = t0 + ttl / 1000.0
        if gone:
            self.bank.clear(np.array(gone, np.uint32))
        if have:
            self.bank.import_redis(np.array(have, np.uint32), strings, BF_IMPORT_REPLACE)

    def to_redis_string(self, name) -> bytes:
        return self.bank.export_redis(np.array([self._id(name)], np.uint32))[0]

    def close(self) -> None:
        self.bank.close()
