"""GPU: every kernel instantiation the library can launch is launched once and compared with the
oracle (tests/census_cases.py holds the families, the generators and the lists of exceptions).

One parametrized test per family runs the family's generated cases under ``fir_hip.launch_log()``;
every call is compared bit for bit with the C oracle inside its case.  After its calls the family
asserts that the set of instantiations it launched equals the census restricted to that family minus
UNREACHED, so an instantiation a dispatcher change makes unreachable, or a new one no case reaches,
fails here by name.  The last test fails when the census holds a kernel no family claims or a family
has no generator.
"""
from __future__ import annotations

import pytest

import census_cases as cc
import fir_hip


@pytest.mark.parametrize("family", cc.FAMILIES)
def test_family_launches_its_census(family):
    launched = set()
    for run in cc.cases(family):
        with fir_hip.launch_log() as log:
            run()
        assert log, (family, "a case launched nothing")
        launched |= {cc.key(l) for l in log if cc.family_of(l) == family}
    want = cc.expected(family)
    missing, extra = sorted(want - launched), sorted(launched - want)
    assert not missing, f"{family}: {len(missing)} of {len(want)} instantiations never launched, e.g. {missing[:8]}"
    # launched but listed as impossible: the list is stale
    assert not extra, f"{family}: launched although listed in UNREACHED: {extra[:8]}"


def test_every_census_entry_is_launched_or_stated_unreachable():
    """A new kernel cannot join the library untested: every census entry belongs to a family that
    has a generator (whose test above holds launched == expected) and is either in that family's
    expected set or in UNREACHED; each UNREACHED pattern cites its source line and matches exactly
    the number of entries written beside it."""
    census = fir_hip.kernel_census()
    assert sorted(cc.GENERATED) == sorted(cc.FAMILIES), sorted(set(cc.FAMILIES) - set(cc.GENERATED))
    orphans = sorted({cc.key(l) for l in census if cc.family_of(l) is None})
    assert not orphans, f"kernels in the library that no census family claims: {orphans[:8]}"
    for pattern, why in cc.UNREACHED.items():
        n = sum(cc.listed(cc.key(l), {pattern: why}) for l in census)
        assert n == cc.UNREACHED_COUNT[pattern], (pattern, n, cc.UNREACHED_COUNT[pattern])
        assert ".h:" in why or ".hip:" in why or ".hip " in why, f"UNREACHED[{pattern!r}] must cite the source line that forbids it"
    held = set().union(*(cc.expected(f) for f in cc.FAMILIES))  # what the family tests above hold launched
    for l in census:
        k = cc.key(l)
        assert (k in held) != cc.listed(k, cc.UNREACHED), k
    assert sum(cc.UNREACHED_COUNT.values()) == sum(cc.listed(cc.key(l), cc.UNREACHED) for l in census)
