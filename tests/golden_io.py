"""Loader of the MPICH golden vectors, tests/golden/golden_np<N>_p<k>.npz (test fixtures, data
only).  tests/golden/make_golden.py writes one team size's cases over as many part files as keep
each below the repository's size limit for a committed file; the parts hold disjoint cases."""
from __future__ import annotations

from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"


def golden_parts(npes: int) -> list[Path]:
    return sorted(GOLDEN.glob(f"golden_np{npes}_p*.npz"))


def load_golden(npes: int) -> dict[str, np.ndarray] | None:
    """Every array of the team size's golden cases (<case>__meta / __in / __out), or None when no
    golden vectors exist for this team size."""
    parts = golden_parts(npes)
    if not parts:
        return None
    out: dict[str, np.ndarray] = {}
    for p in parts:
        with np.load(p) as z:
            for k in z.files:
                if k in out:
                    raise RuntimeError(f"golden array {k} is in more than one part file ({p.name})")
                out[k] = z[k]
    return out
