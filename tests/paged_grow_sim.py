"""A pure-Python model of ContinuousBatcher(reserve="grow") for the tests: the step loop of serving.py on counters
instead of tensors -- growth, preemption of the newest, the swapped queue, admission with headroom, retirement -- built on the same
`paging` functions.  It checks its own invariants at every step (pages are conserved; a request in flight holds exactly
ceil(rows_next / 64) pages) and returns a trace the GPU tests compare the real batcher with."""
import collections

from videollama2_amd.paging import admit_grow, pages_for, pages_needed, plan_growth, rows_next


class Req:
    def __init__(self, rid, S, budget, stop, max_seq_len):
        self.rid, self.S = rid, S
        self.max_new = min(budget, max_seq_len - S + 1)
        self.stop = min(stop, self.max_new)                  # the tokens it really emits (EOS / a stopping criterion)
        self.tokens, self.pages, self.order, self.slot, self.swapped = 0, 0, None, None, False


def simulate(requests, n_pages, max_slots, max_seq_len, arrivals=None, max_steps=100000):
    """requests: [(S, budget, stop)]; arrivals: the step index at which each is submitted (default: all before step 0).  Returns a dict:
    steps, preemptions, resumes, victims (request ids in order), in_flight (requests holding a slot in each step), held ({rid: pages} per
    step, before the step runs), finish (rid -> step of its last token)."""
    reqs = [Req(i, S, b, st, max_seq_len) for i, (S, b, st) in enumerate(requests)]
    for r in reqs:
        assert pages_needed(r.S, r.max_new, max_seq_len) <= n_pages - 1, "submit refuses a request whose worst case exceeds the pool"
    arrivals = [0] * len(reqs) if arrivals is None else list(arrivals)
    pending = sorted(zip(arrivals, range(len(reqs))))
    waiting, swapped = collections.deque(), collections.deque()
    slots, free, orders = [None] * max_slots, n_pages - 1, 0
    out = dict(steps=0, preemptions=0, resumes=0, victims=[], in_flight=[], held=[], finish={}, resumed_elsewhere=0)
    step = 0
    while pending or waiting or swapped or any(r is not None for r in slots):
        assert step < max_steps, "the schedule does not drain"
        while pending and pending[0][0] <= step:
            waiting.append(reqs[pending.pop(0)[1]])
        live = {r.order: r for r in slots if r is not None}
        grants, victims = plan_growth([(o, r.pages, rows_next(r.S, r.tokens, max_seq_len)) for o, r in live.items()], free)
        for o in victims:
            r = live[o]
            free += r.pages
            slots[r.slot] = None
            r.swapped = True
            swapped.append(r)
            swapped = collections.deque(sorted(swapped, key=lambda q: q.order))
            out["preemptions"] += 1
            out["victims"].append(r.rid)
        for o, n in grants:
            assert n <= free
            free -= n
            live[o].pages += n
        if not victims:
            queue = list(swapped) + list(waiting)
            needs = [pages_for(rows_next(r.S, r.tokens, max_seq_len)) for r in queue]
            empty = [s for s, r in enumerate(slots) if r is None]
            take = admit_grow(needs, len(empty), free, max_slots - len(empty))
            for r, need, slot in zip(queue[:take], needs, empty):
                (swapped if r.swapped else waiting).popleft()
                assert need <= free
                free -= need
                if r.swapped:
                    assert need in (r.pages, r.pages + 1)
                    out["resumes"] += 1
                    out["resumed_elsewhere"] += slot != r.slot
                    r.swapped = False
                else:
                    r.order, orders = orders, orders + 1
                r.pages, r.slot = need, slot
                slots[slot] = r
        running = [r for r in slots if r is not None]
        if not running:                                    # nothing submitted yet
            step += 1
            continue
        assert free + sum(r.pages for r in running) == n_pages - 1, "pages are not conserved"
        for r in running:
            assert r.pages == pages_for(rows_next(r.S, r.tokens, max_seq_len)), (r.rid, r.pages)
            assert r.pages <= pages_needed(r.S, r.max_new, max_seq_len)
        assert min(r.order for r in running) == min([r.order for r in running] + [r.order for r in swapped]), "the oldest was preempted"
        out["in_flight"].append(len(running))
        out["held"].append({r.rid: r.pages for r in running})
        for r in running:
            r.tokens += 1
            if r.tokens >= r.stop:
                out["finish"][r.rid] = step
                free += r.pages
                slots[r.slot] = None
        step += 1
        out["steps"] += 1
    assert free == n_pages - 1
    return out
