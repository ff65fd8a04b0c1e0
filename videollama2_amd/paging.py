"""Host side of the paged KV cache (kernels: csrc/k_attn_paged.h): the page allocator, a request's reservation and the
admission rule of the continuous batcher.  Pure Python: nothing here touches a device, so `decoder.py` and `serving.py` share it and the
CPU tests call it without a decoder.

A page is 64 consecutive positions of one sequence (all kv heads, every layer, K and V: one id names them all).  Page 0 is the PARKING page:
it is never handed out, and the table row of a slot that holds no request points its entry 0 at it, so that a step computed for such a slot
at position 0 reads and writes finite, harmless rows.

A resident prefix (kernels: csrc/k_attn_paged_shared.h) shares the WHOLE pages of a prompt prefix among the requests of a
batcher: `shared_rows`, a request's own reservation `own_pages_needed` and the row of an empty slot behind the prefix, `prefix_parked_row`.

Reservations that grow page by page (`ContinuousBatcher(reserve="grow")`): `rows_next`, the rows a request needs a
page for before its next step; `plan_growth`, one step's grants and the requests preempted to serve them; `admit_grow`, admission on the
pages of the prompt with headroom."""

PAGE_ROWS = 64
PARKING_PAGE = 0


def pages_needed(S, max_new, max_seq_len):
    """Pages a request of S prompt rows that may feed max_new tokens reserves: ceil(min(S + max_new, max_seq_len) / 64) -- every row it
    can write before it retires, the cache end included."""
    rows = min(int(S) + int(max_new), int(max_seq_len))
    return (rows + PAGE_ROWS - 1) // PAGE_ROWS


def table_row(pages, pages_per_seq):
    """A request's row of the page table as a list: its pages in position order, -1 behind them."""
    if len(pages) > pages_per_seq:
        raise ValueError(f"{len(pages)} pages do not fit a table row of {pages_per_seq}")
    return list(pages) + [-1] * (pages_per_seq - len(pages))


def parked_row(pages_per_seq):
    """The row of a slot that holds no request: entry 0 = the parking page, the rest not assigned."""
    return table_row([PARKING_PAGE], pages_per_seq)


def shared_rows(P):
    """Rows of a P-row prefix that a resident prefix shares: its WHOLE pages, 64 * floor(P / 64).  The ragged tail
    P - shared_rows(P) (0 .. 63 rows) is prepended to every request's suffix."""
    return int(P) // PAGE_ROWS * PAGE_ROWS


def own_pages_needed(P, n, max_new, max_seq_len):
    """Pages a request of n suffix rows behind a resident prefix of P rows reserves for itself: every page of its P + n prompt rows and its
    new tokens that is not one of the prefix's whole pages."""
    return pages_needed(int(P) + int(n), max_new, max_seq_len) - int(P) // PAGE_ROWS


def prefix_parked_row(prefix_pages, pages_per_seq):
    """The row of a slot that holds no request while a prefix is resident: the prefix pages, then the parking page, then not assigned -- a
    step computed for such a slot at position shared_rows(P) reads the prefix and reads and writes row 0 of page 0."""
    return table_row(list(prefix_pages) + [PARKING_PAGE], pages_per_seq)


class PagePool:
    """The free list over pages 1 .. n_pages - 1 (page 0 is the parking page).  Deterministic: `alloc` hands out the lowest free ids first, so
    a run repeats its page placement."""

    def __init__(self, n_pages):
        n_pages = int(n_pages)
        if n_pages < 1:
            raise ValueError(f"PagePool: n_pages {n_pages}: the pool holds at least the parking page")
        self.n_pages = n_pages
        self._free = set(range(1, n_pages))

    @property
    def n_free(self):
        return len(self._free)

    def alloc(self, n):
        """n page ids, lowest free first.  Raises (and takes none) if fewer than n are free."""
        n = int(n)
        if n < 0:
            raise ValueError(f"PagePool.alloc: {n} pages")
        if n > len(self._free):
            raise RuntimeError(f"PagePool.alloc: {n} pages needed, {len(self._free)} free (of {self.n_pages - 1})")
        ids = sorted(self._free)[:n]
        self._free.difference_update(ids)
        return ids

    def free(self, ids):
        """Give pages back.  Page 0, an id outside the pool, an id that is free already and a repeated id are refused, and then none is freed."""
        ids = [int(i) for i in ids]
        for i in ids:
            if i == PARKING_PAGE:
                raise ValueError("PagePool.free: page 0 is the parking page, it is never handed out")
            if not 0 < i < self.n_pages:
                raise ValueError(f"PagePool.free: page {i} is not of this pool (1 .. {self.n_pages - 1})")
            if i in self._free:
                raise ValueError(f"PagePool.free: page {i} is free already (double free)")
        if len(set(ids)) != len(ids):
            raise ValueError(f"PagePool.free: a page is named twice in {ids} (double free)")
        self._free.update(ids)


def rows_next(S, n_tokens, max_seq_len):
    """Rows that must have a page before the next step of a request of S prompt rows that has emitted n_tokens: min(S + n_tokens + 1,
    max_seq_len).  Step k emits token k and writes row S + k, so ceil(rows_next(S, max_new - 1, ...) / 64) == pages_needed(S, max_new, ...):
    a request that grows page by page ends on its whole reservation and never exceeds it."""
    return min(int(S) + int(n_tokens) + 1, int(max_seq_len))


def pages_for(rows):
    """Pages that hold `rows` rows: ceil(rows / 64)."""
    return (int(rows) + PAGE_ROWS - 1) // PAGE_ROWS


def plan_growth(in_flight, free_pages):
    """The growth and preemption decision of one step under reserve="grow" (DESIGN.md section 23).  in_flight: (admission order, pages held,
    rows_next) per request in flight, any order; free_pages: what the pool holds.  Every request must hold ceil(rows_next / 64) pages before
    the step.  Grants go oldest first; when the pool cannot serve a grant the NEWEST admitted request still in flight is taken as a victim
    (possibly the requester itself): its pages count as free and its own grant is dropped.  No victim is taken while the free pages suffice,
    and the oldest request is never one: a pool that cannot serve it alone raises RuntimeError (`submit` refuses such a request).
    Returns (grants, victims): grants = [(admission order, pages to add > 0)] oldest first, victims = [admission order] newest first."""
    alive = sorted((int(o), int(held), max(0, pages_for(rows) - int(held))) for o, held, rows in in_flight)
    free = int(free_pages)
    grants, victims = [], []
    i = 0
    while i < len(alive):
        order, held, want = alive[i]
        if want <= free:
            free -= want
            if want:
                grants.append((order, want))
            i += 1
            continue
        if len(alive) == 1:
            raise RuntimeError(f"plan_growth: the oldest request holds {held} pages and needs {want} more, the pool has {free} free with "
                               f"nobody left to preempt")
        v_order, v_held, _ = alive.pop()        # the newest admitted; i itself when it is the last one alive (then the loop ends)
        victims.append(v_order)
        free += v_held
    return grants, victims


def admit_grow(queue_needs, free_slots, free_pages, n_in_flight):
    """Admission of one step under reserve="grow".  queue_needs: the pages each queued request must get NOW, in queue order (a new request:
    ceil(rows_next / 64) of its prompt; a resumed one: the same of its position, i.e. its saved pages, plus one at a page edge).  Strict FIFO:
    the head joins only if a slot is free, the pool holds its pages, and afterwards one free page per request then in flight (itself
    included) remains as headroom -- so that admission does not cause the next step's preemption.  The headroom rule is waived for a step
    that begins with nothing in flight (n_in_flight == 0): an idle batcher fills its slots on the pages of the prompts alone, and a request
    that fills the pool alone can start.  Returns how many requests from the head are admitted."""
    n = 0
    free_slots, free_pages, n_in_flight = int(free_slots), int(free_pages), int(n_in_flight)
    headroom = n_in_flight > 0
    for need in queue_needs:
        if free_slots <= 0 or need > free_pages:
            break
        if headroom and free_pages - need < n_in_flight + 1:
            break
        free_slots -= 1
        free_pages -= need
        n_in_flight += 1
        n += 1
    return n


def admit_fifo(needs, free_slots, free_pages):
    """The continuous batcher's admission decision for one step.  needs: the reservations (pages) of the waiting requests in submission
    order; free_slots / free_pages: what the step has to give.  Strict FIFO: the head of the queue is admitted only when a slot is free AND
    the pool holds its whole reservation; otherwise admission stops for this step -- nobody behind it is admitted, however small.
    Returns how many requests from the head of the queue are admitted."""
    n = 0
    for need in needs:
        if free_slots <= 0 or need > free_pages:
            break
        free_slots -= 1
        free_pages -= need
        n += 1
    return n
