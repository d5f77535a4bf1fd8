"""An independent check of a conv-net plan's workspace layout and lane ordering (``kvq_convnet_layout``), in plain Python.

It shares no code with the planner of csrc/convnet.hip: it is handed the finished tables and decides from them alone whether a
forward of the plan can damage a live value or race.  A layout is a dict

    ws_bytes   the workspace size the plan asks for
    scratch    [(offset, bytes)] per lane: that lane's split-K scratch
    slots      [(offset, bytes, in_workspace)]
    ops        [{"lane": l, "reads": [slot..], "writes": [slot..], "wait": op index or -1}] in program (enqueue) order

``check(layout)`` returns the list of defects, each a sentence that names the slots / ops involved; an empty list is a pass.

1. Every slot and every scratch range lies inside the workspace, no slot overlaps a scratch range, and the scratch ranges of the
   lanes do not overlap each other.
2. A slot is live from the first op that writes it to the last op that touches it.  Two slots whose bytes overlap must have
   disjoint live intervals; a workspace slot must not be read before an op has written it.
3. Ops of different lanes that touch overlapping bytes, at least one of them writing, must be ordered: the earlier op (program
   order) has to happen before the later one in the transitive closure of same-lane program order and the wait edges
   (``wait`` = the op whose completion event the op's stream waits for before the op starts).
"""


def _overlap(a, b):
    return a[0] < b[0] + b[1] and b[0] < a[0] + a[1]


def live_intervals(layout):
    """{slot: (first op writing it, last op touching it)} of the workspace slots some op writes"""
    first, last = {}, {}
    for i, op in enumerate(layout["ops"]):
        for s in op["writes"]:
            first.setdefault(s, i)
        for s in list(op["reads"]) + list(op["writes"]):
            last[s] = i
    return {s: (first[s], last[s]) for s in first if layout["slots"][s][2]}


def happens_before(layout):
    """anc[j] = bit mask of the ops known to have finished when op j starts"""
    ops = layout["ops"]
    anc, prev_in_lane = [0] * len(ops), {}
    for j, op in enumerate(ops):
        preds = []
        if op["lane"] in prev_in_lane:
            preds.append(prev_in_lane[op["lane"]])
        if op["wait"] >= 0 and op["wait"] < j:          # an event recorded later in program order orders nothing
            preds.append(op["wait"])
        for p in preds:
            anc[j] |= anc[p] | (1 << p)
        prev_in_lane[op["lane"]] = j
    return anc


def check(layout):
    problems = []
    slots, ops, ws_bytes, scratch = layout["slots"], layout["ops"], layout["ws_bytes"], layout["scratch"]
    in_ws = [s for s in range(len(slots)) if slots[s][2]]
    # ---- 1. ranges ------------------------------------------------------------------------------------------------------
    for s in in_ws:
        off, nb, _ = slots[s]
        if off + nb > ws_bytes:
            problems.append(f"slot {s} [{off}, {off + nb}) ends past the workspace of {ws_bytes} bytes")
    for lane, (off, nb) in enumerate(scratch):
        if nb and off + nb > ws_bytes:
            problems.append(f"scratch of lane {lane} [{off}, {off + nb}) ends past the workspace of {ws_bytes} bytes")
        for s in in_ws:
            if nb and slots[s][1] and _overlap(slots[s][:2], (off, nb)):
                problems.append(f"slot {s} [{slots[s][0]}, {slots[s][0] + slots[s][1]}) reaches into the scratch of lane {lane} "
                                f"[{off}, {off + nb})")
        for other in range(lane):
            if nb and scratch[other][1] and _overlap(scratch[other], (off, nb)):
                problems.append(f"scratch of lane {other} overlaps the scratch of lane {lane}")
    # ---- 2. live intervals ----------------------------------------------------------------------------------------------
    live = live_intervals(layout)
    for i, op in enumerate(ops):
        for s in op["reads"]:
            if slots[s][2] and (s not in live or live[s][0] > i):
                problems.append(f"op {i} reads slot {s} before any op has written it")
        if op["wait"] >= i:
            problems.append(f"op {i} waits for op {op['wait']}, which is not enqueued before it")
    placed = sorted(live)
    for x, a in enumerate(placed):
        for b in placed[x + 1:]:
            if slots[a][1] and slots[b][1] and _overlap(slots[a][:2], slots[b][:2]):
                (fa, la), (fb, lb) = live[a], live[b]
                if not (la < fb or lb < fa):
                    problems.append(f"slots {a} and {b} share bytes while both are live (ops {fa}..{la} and {fb}..{lb})")
    # ---- 3. cross-lane ordering -----------------------------------------------------------------------------------------
    anc = happens_before(layout)

    def touches(op):
        return [(s, False) for s in op["reads"] if slots[s][2]] + [(s, True) for s in op["writes"] if slots[s][2]]

    for j, oj in enumerate(ops):
        tj = touches(oj)
        for i in range(j):
            oi = ops[i]
            if oi["lane"] == oj["lane"] or (anc[j] >> i) & 1:
                continue
            hit = next(((a, b) for a, wa in touches(oi) for b, wb in tj
                        if (wa or wb) and slots[a][1] and slots[b][1] and _overlap(slots[a][:2], slots[b][:2])), None)
            if hit:
                problems.append(f"op {i} (lane {oi['lane']}, slot {hit[0]}) and op {j} (lane {oj['lane']}, slot {hit[1]}) touch the same "
                                f"bytes, one of them writing, with no ordering between the lanes")
    return problems
