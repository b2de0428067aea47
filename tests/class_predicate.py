"""The selection predicate of raft_census_select and raft_audit_select on a record's class names
(test infrastructure; tests/census_oracle.py and tests/audit_oracle.py select with it)."""
from __future__ import annotations


def matches(rec, any=(), all=(), none=()):
    """In one of the classes `any` (empty: no such condition), in every class of `all`, in no
    class of `none`."""
    have = set(rec["classes"])
    return ((not any or bool(have & set(any))) and set(all) <= have and not (have & set(none)))
