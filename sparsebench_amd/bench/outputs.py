"""bench.py --dump-outputs DIR: what the timed loop computed in its last step, as DIR/<name>.npy (float64), so that two builds can be
compared output for output.  A caller of solveCG receives x; the CG wrapper also hands out the r.r and p.Ap histories of the solve.
The arrays come from the last segment of the clean timed pass (restarted from x0 = 0 like every segment): with the same arguments
the inputs, and so the outputs, are the same from run to run.  At most MAX_BYTES in all: an array that does not fit is replaced by a
fixed, seeded sample of its entries (`<name>` holds the values, `<name>_sample_index` their positions)."""
import os

MAX_BYTES = 60 << 20   # below the 64 MB the dump may take, leaving room for the .npy headers
SEED = 20260101


def capture(cg):
    """the arrays a caller of the timed loop receives, read after sb_cg_finish (outside every clock)"""
    rr, pap = cg.history()
    return {"x": cg.solution(), "rr_history": rr, "pAp_history": pap}


def write(dirname, arrays, suffix=""):
    """arrays: {name: 1-D float64 array}; returns the list of files written"""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    total = sum(8 * len(v) for v in arrays.values())
    big = [k for k, v in arrays.items() if 8 * len(v) > (MAX_BYTES // max(1, len(arrays)))]
    out = {}
    if total > MAX_BYTES and big:
        small = sum(8 * len(v) for k, v in arrays.items() if k not in big)
        keep = max(1, (MAX_BYTES - small) // (len(big) * 16))  # value + its position, 8 B each
        rng = np.random.default_rng(SEED)
        for k, v in arrays.items():
            if k in big and len(v) > keep:
                idx = np.sort(rng.choice(len(v), size=keep, replace=False))
                out[k] = np.asarray(v, dtype=np.float64)[idx]
                out[k + "_sample_index"] = idx.astype(np.float64)
            else:
                out[k] = np.asarray(v, dtype=np.float64)
    else:
        out = {k: np.asarray(v, dtype=np.float64) for k, v in arrays.items()}
    files = []
    for k, v in out.items():
        path = os.path.join(dirname, k + suffix + ".npy")
        np.save(path, v)
        files.append(path)
    return files
