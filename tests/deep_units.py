"""Data units whose luma AC symbol counts are hufopt_model.deep_counts(depth): a code tree that is one chain, `depth` bits deep
before K.3's shortening.  Depth 17-32 exercises the shortening, depth 33 the fall-back to the plain tables."""
import ctypes as C

import numpy as np

import hufopt_model as hm


def _value(n):
    return 1 << (n - 1)  # the smallest value of magnitude category n


def deep_chain_units(ica, depth, quality=90):
    """-> (plan, du [n, 64] int16) of a 4:2:0 picture.  The `depth` symbols are run/size pairs: the ten largest counts go to run 0
    (sizes 1-10), the others to runs 1-3.  Every luma unit is filled up to coefficient 63 (no EOB, no ZRL) with the symbol of the
    largest count, which may so exceed its count -- the chain only needs it above the sum of the others.  Chroma units are zero."""
    c = hm.deep_counts(depth)
    n0 = min(10, depth)
    fill_val, fills, units = _value(n0), 0, []
    for k in range(depth - n0):  # runs 1..3: whole units of one symbol, the rest of each unit filled
        r, n = 1 + k // 10, 1 + k % 10
        per = 63 // (r + 1)
        for reps, items in ((c[k] // per, per), (1 if c[k] % per else 0, c[k] % per)):
            if reps:
                u = np.zeros(64, np.int16)
                u[(r + 1) * np.arange(1, items + 1)] = _value(n)
                u[items * (r + 1) + 1:] = fill_val
                fills += reps * (63 - items * (r + 1))
                units.append(np.repeat(u[None], reps, axis=0))
    seq = np.repeat(np.array([_value(n) for n in range(1, n0)], np.int16), c[depth - n0:depth - 1])  # run 0, all but the largest
    pad = -len(seq) % 63
    fills += pad
    seq = np.concatenate([seq, np.full(pad, fill_val, np.int16)]).reshape(-1, 63)
    units.append(np.concatenate([np.zeros((len(seq), 1), np.int16), seq], axis=1))
    luma = sum(len(u) for u in units) + max(0, -(-(c[-1] - fills) // 63))
    n_mcu = -(-luma // 4)
    mcu_x = min(n_mcu, 256)
    mcu_y = -(-n_mcu // mcu_x)
    full = np.full(64, fill_val, np.int16)
    full[0] = 0
    units.append(np.repeat(full[None], mcu_x * mcu_y * 4 - sum(len(u) for u in units), axis=0))
    du = np.zeros((mcu_x * mcu_y, 6, 64), np.int16)
    du[:, :4] = np.concatenate(units).reshape(-1, 4, 64)
    plan = ica.binding.WritePlan()
    L = ica.lib()
    L.mjw_plan_init.argtypes = [C.POINTER(ica.binding.WritePlan), C.c_int, C.c_int, C.c_int, C.c_int]
    assert L.mjw_plan_init(C.byref(plan), 16 * mcu_x, 16 * mcu_y, 3, quality) and plan.du_per_mcu == 6
    return plan, du.reshape(-1, 64)
