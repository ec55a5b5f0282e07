"""newpoint_map on the device, restated in plain Python / NumPy: the rules of the "front end: newpoint_map on the device" block of include/scavislam_hip.h.
tests/test_newpoint_cpu.py holds this model to a literal restatement of stereo_frontend.cpp:360-365, :808 and :989-1029; tests/test_gpu_newpoints.py holds the
library to this model, byte for byte."""
import numpy as np

from scavislam_amd.ctypes_types import CANDIDATE_DTYPE

MATCH_OK = 0
PREPEND, REPLACE = 0, 1
MAX_GROUPS = 64


class Refused(Exception):
    """a call the library refuses with nothing changed; .status = SVS_ERR_INVALID (1) or SVS_ERR_CAPACITY (4)"""

    def __init__(self, status):
        super().__init__(f"status {status}")
        self.status = status


def prune_set(res, gated, pts, n_new):
    """rule 4's P: the point_id of every record i of the step with status OK, accepted and i < the list's new-record count"""
    n = min(len(res), max(int(n_new), 0))
    ok = (res["status"][:n] == MATCH_OK) & (gated["accepted"][:n] != 0)
    return set(int(p) for p in pts["point_id"][:n][ok])


class Store:
    """one stream's store: groups in creation order, each (key, records in list order)"""

    def __init__(self, record_cap, group_cap=MAX_GROUPS):
        self.record_cap, self.group_cap = int(record_cap), int(group_cap)
        self.keys, self.groups = [], []

    def copy(self):
        s = Store(self.record_cap, self.group_cap)
        s.keys, s.groups = list(self.keys), [g.copy() for g in self.groups]
        return s

    def total(self):
        return sum(len(g) for g in self.groups)

    def _group(self, key):
        if key < 0:
            raise Refused(1)
        if key not in self.keys:
            if len(self.keys) >= self.group_cap:
                raise Refused(4)
            self.keys.append(int(key))
            self.groups.append(np.zeros(0, CANDIDATE_DTYPE))
        return self.keys.index(key)

    def put(self, key, records, mode=PREPEND):
        """rule 2 (and rule 3 with the seeded records); all or nothing"""
        records = np.asarray(records, CANDIDATE_DTYPE).reshape(-1)
        if mode not in (PREPEND, REPLACE):
            raise Refused(1)
        t = self.copy()
        g = t._group(key)
        t.groups[g] = records.copy() if mode == REPLACE else np.concatenate([records, t.groups[g]])
        if t.total() > self.record_cap:
            raise Refused(4)
        self.keys, self.groups = t.keys, t.groups

    def put_all(self, requests):
        """several requests of one call: in order, and the stream stays as it was when any of them is refused"""
        t = self.copy()
        for q in requests:
            t.put(q["kf_id"], q.get("records", np.zeros(0, CANDIDATE_DTYPE)), q.get("mode", PREPEND))
        self.keys, self.groups = t.keys, t.groups

    def prune(self, P):
        """rule 4: returns (n_removed, counts)"""
        before = self.total()
        self.groups = [g[~np.isin(g["point_id"], sorted(P))] if len(P) else g for g in self.groups]
        return before - self.total(), [len(g) for g in self.groups]

    def drop(self, keys):
        """rule 5: returns n_found"""
        found = 0
        for k in keys:
            if k in self.keys:
                i = self.keys.index(k)
                del self.keys[i], self.groups[i]
                found += 1
        return found

    def records(self):
        return np.concatenate(self.groups) if self.groups else np.zeros(0, CANDIDATE_DTYPE)

    def table_rows(self):
        """(n_groups, keys [64] with -1 behind the groups, counts [64] with 0 behind them): the device's table"""
        keys, counts = np.full(MAX_GROUPS, -1, np.int32), np.zeros(MAX_GROUPS, np.int32)
        keys[:len(self.keys)] = self.keys
        counts[:len(self.keys)] = [len(g) for g in self.groups]
        return len(self.keys), keys, counts

    def compose(self, keys, slot_kf, tail, max_points):
        """rule 6: (records, group_end, result dict) -- records None when the list does not fit (rule 7)"""
        keys = [int(k) for k in keys]
        if not 1 <= len(keys) or any(k < 0 for k in keys) or len(set(keys)) != len(keys):
            raise Refused(1)
        if len(keys) > MAX_GROUPS - 1:
            raise Refused(4)
        slot_kf = [int(s) for s in slot_kf]
        tail = np.asarray(tail, CANDIDATE_DTYPE).reshape(-1)
        parts, ends, n_no_slot = [], [], 0
        for k in keys:
            g = self.groups[self.keys.index(k)].copy() if k in self.keys else np.zeros(0, CANDIDATE_DTYPE)
            g["kf_index"] = slot_kf.index(k) if k in slot_kf else -1
            n_no_slot += len(g) if k not in slot_kf else 0
            parts.append(g)
            ends.append(sum(len(p) for p in parts))
        n_head = ends[-1]
        res = dict(n_points=n_head + len(tail), n_head=n_head, n_groups=len(keys) + 1, n_no_slot=n_no_slot, over_capacity=0)
        if res["n_points"] > max_points:
            res.update(over_capacity=1, n_no_slot=0)
            return None, None, res
        return np.concatenate(parts + [tail]), ends + [n_head + len(tail)], res


def random_records(rng, n, first_id, kf_index=0):
    r = np.zeros(n, CANDIDATE_DTYPE)
    r["xyz_anchor"], r["anchor_obs_pyr"] = rng.normal(size=(n, 3)), rng.uniform(0, 500, size=(n, 3))
    r["anchor_level"], r["kf_index"], r["point_id"] = rng.integers(0, 3, n), kf_index, first_id + np.arange(n)
    return r
