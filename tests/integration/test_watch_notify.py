"""kube-lite's watch delivery after the notify rule changed: a commit wakes a watch writer
only when the writer's queue becomes non-empty, reaches the burst threshold (16) or
overflows, and a batch is framed once into one chunk.

Every watch must still receive every event it should, exactly once and in order, whatever
the coalescing window; no wake-up may be lost (nothing here may lean on the writer's
500 ms backstop wait); and the counters in /_kl/stats must show the rule at work."""
import http.client
import json
import threading
import time
from urllib.parse import urlsplit

import pytest
import requests

from bacchus_gpu_controller_amd.testing.cluster import ADMIN_TOKEN, Cluster
from bacchus_gpu_controller_amd.testing.kubeapi import KubeApi

pytestmark = pytest.mark.slow

AUTH = {"Authorization": f"Bearer {ADMIN_TOKEN}"}
META_ACCEPT = "application/json;as=PartialObjectMetadata;g=meta.k8s.io;v=v1"
WRITERS, PER_WRITER = 8, 40
SENTINEL = "zz-end"


@pytest.fixture(scope="module")
def c():
    with Cluster(admission=False, controller=False) as cl:
        yield cl


@pytest.fixture(scope="module")
def c_long():
    """A kube-lite whose coalescing window is 200000 us (beyond what POST /_kl/watch-coalesce-us
    accepts, so it is set at start-up)."""
    with Cluster(admission=False, controller=False, apiserver_args=["--watch-coalesce-us", "200000"]) as cl:
        yield cl


def set_coalesce(c, us):
    r = requests.post(c.server + "/_kl/watch-coalesce-us", data=str(us), headers=AUTH, timeout=5)
    assert r.status_code == 200
    return int(r.text)


def make_ns(c, name):
    c.admin.create("namespaces", {"apiVersion": "v1", "kind": "Namespace", "metadata": {"name": name}})


def configmap(name, labels=None, data=None):
    meta = {"name": name}
    if labels:
        meta["labels"] = labels
    return {"apiVersion": "v1", "kind": "ConfigMap", "metadata": meta, "data": data or {"k": "0"}}


class Watcher(threading.Thread):
    """Streams one watch and keeps (arrival time, raw line) of every event up to and including
    the one named `until` (or until the server ends the stream)."""

    def __init__(self, c, ns, rv, accept=None, selector=None, until=SENTINEL, seconds=30):
        super().__init__(daemon=True)
        u = urlsplit(c.server)
        self.conn = http.client.HTTPConnection(u.hostname, u.port, timeout=seconds + 5)
        q = f"/api/v1/namespaces/{ns}/configmaps?watch=1&resourceVersion={rv}&timeoutSeconds={seconds}"
        if selector:
            q += "&labelSelector=" + selector
        headers = dict(AUTH)
        if accept:
            headers["Accept"] = accept
        self.conn.request("GET", q, headers=headers)
        self.resp = self.conn.getresponse()
        assert self.resp.status == 200
        self.until = until
        self.lines = []  # (monotonic seconds, bytes)
        self.arrived = {}  # object name -> arrival time of its first event
        self.cond = threading.Condition()
        self.start()

    def run(self):
        try:
            while True:
                line = self.resp.readline()
                if not line:
                    return
                now = time.monotonic()
                name = json.loads(line)["object"]["metadata"].get("name")
                with self.cond:
                    self.lines.append((now, line))
                    self.arrived.setdefault(name, now)
                    self.cond.notify_all()
                if name == self.until:
                    return
        finally:
            self.conn.close()

    def wait_for_names(self, names, timeout):
        """Arrival times of `names`, waiting up to `timeout` s for the last of them."""
        deadline = time.monotonic() + timeout
        with self.cond:
            while not all(n in self.arrived for n in names):
                left = deadline - time.monotonic()
                assert left > 0, f"events missing after {timeout} s: {[n for n in names if n not in self.arrived]}"
                self.cond.wait(left)
            return [self.arrived[n] for n in names]

    def events(self):
        return [json.loads(line) for _, line in self.lines]


def key(ev):
    m = ev["object"]["metadata"]
    return ev["type"], m["name"], int(m["resourceVersion"])


def raw_value(text, at):
    """The JSON value starting at text[at] (an object or a string), as raw text."""
    depth, i, in_str = 0, at, False
    while True:
        ch = text[i]
        if in_str:
            if ch == "\\":
                i += 1
            elif ch == '"':
                in_str = False
                if depth == 0:
                    return text[at:i + 1]
        elif ch == '"':
            in_str = True
        elif ch in "{[":
            depth += 1
        elif ch in "}]":
            depth -= 1
            if depth == 0:
                return text[at:i + 1]
        i += 1


def partial_metadata_line(line):
    """What a metadata-only watch receives for the full event line `line`, byte for byte."""
    text = line.decode()
    type_at = text.index('"type":') + len('"type":')
    obj_at = text.index('"object":') + len('"object":')
    obj = raw_value(text, obj_at)
    md = raw_value(obj, obj.index('"metadata":') + len('"metadata":'))
    return ('{"type":' + raw_value(text, type_at) +
            ',"object":{"kind":"PartialObjectMetadata","apiVersion":"meta.k8s.io/v1","metadata":' + md + "}}\n").encode()


def churn(c, ns, w, written):
    """One writer: creates, patches and deletes its ConfigMaps.  The first patch moves the
    object into the selector `sel=in`, the third moves every second object out again."""
    api = KubeApi(c.server, ADMIN_TOKEN)
    mine = []
    for i in range(PER_WRITER):
        name = f"cm-{w}-{i}"
        mine.append(("ADDED", name, int(api.create("configmaps", configmap(name), namespace=ns)["metadata"]["resourceVersion"])))
        patches = [{"metadata": {"labels": {"sel": "in"}}}, {"data": {"k": "1"}}]
        if i % 2 == 0:
            patches.append({"metadata": {"labels": {"sel": None}}})
        for p in patches:
            out = api.merge_patch("configmaps", name, p, namespace=ns)
            mine.append(("MODIFIED", name, int(out["metadata"]["resourceVersion"])))
        api.delete("configmaps", name, namespace=ns)
    written.extend(mine)


@pytest.mark.parametrize("coalesce_us", [0, 50, 20000])
def test_every_watch_gets_every_event_once_in_order(c, coalesce_us):
    ns = f"fan{coalesce_us}"
    make_ns(c, ns)
    prev = set_coalesce(c, coalesce_us)
    try:
        rv = c.admin.list("configmaps", namespace=ns)["metadata"]["resourceVersion"]
        full = Watcher(c, ns, rv)
        meta = Watcher(c, ns, rv, accept=META_ACCEPT)
        sel = Watcher(c, ns, rv, selector="sel%3Din")
        written = []
        threads = [threading.Thread(target=churn, args=(c, ns, w, written)) for w in range(WRITERS)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(60)
        c.admin.create("configmaps", configmap(SENTINEL, labels={"sel": "in"}), namespace=ns)
        for w in (full, meta, sel):
            w.join(20)
            assert not w.is_alive() and w.events()[-1]["object"]["metadata"]["name"] == SENTINEL
    finally:
        set_coalesce(c, prev)

    events = full.events()[:-1]
    keys = [key(e) for e in events]
    rvs = [k[2] for k in keys]
    assert all(a < b for a, b in zip(rvs, rvs[1:])), "resourceVersions must strictly increase"
    # every write the writers saw answered, once, plus one DELETED per object after its last write
    n_objs = WRITERS * PER_WRITER
    assert len(written) == n_objs * 3 + n_objs // 2
    assert sorted(k for k in keys if k[0] != "DELETED") == sorted(written)
    deleted = [k for k in keys if k[0] == "DELETED"]
    assert sorted(k[1] for k in deleted) == sorted({k[1] for k in written})
    last_write = {}
    for _, name, v in written:
        last_write[name] = max(v, last_write.get(name, 0))
    assert all(v > last_write[name] for _, name, v in deleted)

    # metadata-only: the same events, each line the PartialObjectMetadata form of the full one
    assert [line for _, line in meta.lines] == [partial_metadata_line(line) for _, line in full.lines]

    # selector watch: what the full stream implies for sel=in (into the selector = ADDED, out
    # of it = DELETED at the event's resourceVersion, inside it = as it is)
    inside, expected = set(), []
    for ev in events:
        typ, name, v = key(ev)
        now_in = typ != "DELETED" and (ev["object"]["metadata"].get("labels") or {}).get("sel") == "in"
        was_in = name in inside
        if now_in and not was_in:
            expected.append(("ADDED", name, v))
        elif was_in and not now_in:
            expected.append(("DELETED", name, v))
        elif now_in:
            expected.append((typ, name, v))
        (inside.add if now_in else inside.discard)(name)
    assert [key(e) for e in sel.events()[:-1]] == expected
    assert sum(1 for k in expected if k[0] == "ADDED") == n_objs and sum(1 for k in expected if k[0] == "DELETED") == n_objs


def settle(watchers, c, ns, name):
    """One event every watcher has received: their queues are empty and they are back in
    their idle wait before the timed part begins."""
    c.admin.create("configmaps", configmap(name), namespace=ns)
    for w in watchers:
        w.wait_for_names([name], 5)


@pytest.mark.parametrize("coalesce_us", [0, 50])
def test_isolated_events_are_not_held_back(c, coalesce_us):
    """40 isolated commits 20 ms apart: each reaches the watch within 250 ms, well inside the
    writer's 500 ms backstop, so the wake-up for an empty queue turning non-empty was sent."""
    ns = f"iso{coalesce_us}"
    make_ns(c, ns)
    prev = set_coalesce(c, coalesce_us)
    try:
        rv = c.admin.list("configmaps", namespace=ns)["metadata"]["resourceVersion"]
        w = Watcher(c, ns, rv)
        settle([w], c, ns, "warm")
        sent = {}
        for i in range(40):
            name = f"iso-{i}"
            sent[name] = time.monotonic()
            c.admin.create("configmaps", configmap(name), namespace=ns)
            time.sleep(0.02)
        arrived = w.wait_for_names(list(sent), 5)
        delays = [a - sent[n] for n, a in zip(sent, arrived)]
        print("coalesce_us", coalesce_us, "max delay ms", round(max(delays) * 1e3, 2))
        assert max(delays) <= 0.250
        c.admin.create("configmaps", configmap(SENTINEL), namespace=ns)
        w.join(10)
    finally:
        set_coalesce(c, prev)


def burst(c, ns, names):
    """Commits `names` back to back on one warm connection; the time the first was sent."""
    t0 = time.monotonic()
    for n in names:
        c.admin.create("configmaps", configmap(n), namespace=ns)
    return t0


def test_burst_threshold_and_window_end_wake_the_writer(c_long):
    """Window 200000 us.  16 back-to-back events fill the burst threshold: the commit that
    queues the 16th wakes the writer, and all arrive within 100 ms (not after the window).
    3 back-to-back events stay below it: the window's own timer delivers them within 400 ms,
    before the 500 ms backstop.  Over the 16-event burst a watcher is notified at most twice
    (queue non-empty, threshold reached) for its 16 queued events."""
    c = c_long
    ns = "burst"
    make_ns(c, ns)
    rv = c.admin.list("configmaps", namespace=ns)["metadata"]["resourceVersion"]
    watchers = [Watcher(c, ns, rv), Watcher(c, ns, rv, accept=META_ACCEPT)]
    settle(watchers, c, ns, "warm")  # it arrived: the window it opened has ended

    s0 = c.stats()
    names = [f"b16-{i}" for i in range(16)]
    t0 = burst(c, ns, names)
    for w in watchers:
        took = max(w.wait_for_names(names, 5)) - t0
        print("16-event burst arrived after ms", round(took * 1e3, 2))
        assert took <= 0.100
    s1 = c.stats()
    queued = s1["watch_events_queued"] - s0["watch_events_queued"]
    notifies = s1["watch_notifies"] - s0["watch_notifies"]
    batches = s1["watch_batches_written"] - s0["watch_batches_written"]
    print("queued", queued, "notifies", notifies, "batches", batches)
    assert queued == 16 * len(watchers)
    assert notifies <= 2 * len(watchers)
    assert 1 * len(watchers) <= batches <= 2 * len(watchers)

    names = [f"b3-{i}" for i in range(3)]
    t0 = burst(c, ns, names)
    for w in watchers:
        took = max(w.wait_for_names(names, 5)) - t0
        print("3-event burst arrived after ms", round(took * 1e3, 2))
        assert took <= 0.400
    c.admin.create("configmaps", configmap(SENTINEL), namespace=ns)
    for w in watchers:
        w.join(10)
