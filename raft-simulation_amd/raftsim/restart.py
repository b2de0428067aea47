"""Node restarts (SIM_SPEC §4a; include/raftsim.h, "Node restarts") stated in Python.

`restart_record` is the pure restatement of the semantics on one node record and needs no library.
`restart_by_writes` performs the same restart through the read_* / write_* calls of any Backend:
it is the path for the oracle backend (which has no restart entry point) and the reference the
device-side restart of GpuBackend.restart / restart_where is tested against. `supervise` is the
loop a crash-recovery fault model runs: step, restart what has halted, step again.
"""
from __future__ import annotations

from . import _abi
from ._backend import restart_mode

M32 = 0xFFFFFFFF
P_INIT = 1                       # the purpose byte of the INIT draw (SIM_SPEC §4)


def philox(ctr, key):
    """Philox4x32-10 (Random123) of the 4-word counter under the 2-word key: four 32-bit words.
    Passes the known-answer test of SIM_SPEC §5."""
    c0, c1, c2, c3 = (x & M32 for x in ctr)
    k0, k1 = key[0] & M32, key[1] & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def _field(config, name):
    return config[name] if isinstance(config, dict) else getattr(config, name)


def restart_deadline(tick, config, global_id, node_id):
    """The election deadline a restart at `tick` arms node `node_id` of global cluster `global_id`
    with: the INIT draw of SIM_SPEC §4 with the restart tick in the counter's tick word."""
    seed = _field(config, "seed")
    w = philox((global_id, node_id | P_INIT << 8, tick, 0), (seed & M32, seed >> 32))
    return tick + _field(config, "el_base") + ((w[1] * _field(config, "el_span")) >> 32)


def restart_record(node, tick, config, global_id, mode="amnesia", node_id=None):
    """The record (a read_nodes dict) of a node after a restart at `tick`, from its record `node`
    before it. `config` holds el_base, el_span and seed (an _abi.Config or a dict); `node_id` is the
    node's id 1..N (default: node["id"]). Pure: `node` is not changed."""
    durable = restart_mode(mode) == _abi.RESTART_MODES["durable"]
    node_id = node["id"] if node_id is None else node_id
    r = dict(node)
    r.update(role=0, leader_id=0, votes=0, ls_present=0, ls_keys=0, fault=0, commit_index=0,
             entries_is_seq=0, req_count=0, res_count=0,
             next_index=[0] * len(node["next_index"]), match_index=[0] * len(node["match_index"]),
             deadline=restart_deadline(tick, config, global_id, node_id))
    if not durable:
        r.update(current_term=1, voted_for=0, log_len=0, arena_base=node["arena_frontier"])
    return r


def restart_by_writes(backend, cluster, node_ids, mode="amnesia"):
    """Restart the nodes `node_ids` of cluster `cluster` of any Backend at its current tick through
    read_nodes / write_nodes / write_queue(.., []) / read_clusters / write_clusters: what
    GpuBackend.restart does on the device, one synchronous copy at a time. Returns the number of
    nodes restarted."""
    ids = sorted({int(i) for i in node_ids})
    if not ids:
        return 0
    for i in ids:
        if not 1 <= i <= backend.N:
            raise ValueError(f"restart_by_writes: node id {i} outside 1..{backend.N}")
    tick, g = backend.tick, backend.config.cluster_offset + cluster
    recs = backend.read_nodes(cluster, 1)
    for i in ids:
        recs[i - 1] = restart_record(recs[i - 1], tick, backend.config, g, mode, node_id=i)
    backend.write_nodes(cluster, recs)
    for i in ids:
        backend.write_queue(cluster, i, 0, [])
        backend.write_queue(cluster, i, 1, [])
    backend.write_clusters(cluster, backend.read_clusters(cluster, 1))   # the reserved words: zero
    return len(ids)


def supervise(sim, ticks, every, faults=("ioobe", "npe", "cce", "overflow"), mode="amnesia"):
    """Run `sim` (a GpuBackend) for `ticks` ticks under a supervisor that looks every `every`
    ticks and starts the nodes halted with one of `faults` again (restart_where): step, restart,
    step, ... with a restart after every step. Returns the number of nodes restarted per round."""
    if every < 1:
        raise ValueError("supervise: every must be >= 1")
    counts, done = [], 0
    while done < ticks:
        n = min(every, ticks - done)
        sim.step(n)
        done += n
        counts.append(sim.restart_where(faults, mode))
    return counts
