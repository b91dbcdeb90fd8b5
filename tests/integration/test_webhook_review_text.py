"""The AdmissionReview kube-lite sends to a mutating webhook, read by a webhook that records
it: `oldObject` is the stored object exactly as a GET returns it (kube-lite takes its text
from the object's committed event line while the watch history holds it, and dumps the
stored tree once that line has been compacted away), `object` is the write's result before
the server fills in what follows admission, and a denying or unparsable response is turned
into the same status as before the request text was cached."""
import http.server
import json
import os
import ssl
import subprocess
import threading

import pytest

from bacchus_gpu_controller_amd import binary
from bacchus_gpu_controller_amd.testing.cluster import Cluster
from bacchus_gpu_controller_amd.testing.kubeapi import ApiError

pytestmark = pytest.mark.slow

HOOK = "record.bacchus.io"
# what the server fills in after admission (commit): not part of request.object
AFTER_ADMISSION = ("resourceVersion", "managedFields", "generation")


class Recorder:
    """A TLS webhook that keeps every AdmissionReview request and answers by `mode`."""

    def __init__(self, cert_dir):
        self.requests, self.mode, rec = [], "allow", self

        class Handler(http.server.BaseHTTPRequestHandler):
            protocol_version = "HTTP/1.1"

            def do_POST(self):
                review = json.loads(self.rfile.read(int(self.headers["Content-Length"])))
                rec.requests.append(review["request"])
                uid = review["request"]["uid"]
                if rec.mode == "malformed":
                    body = b'{"apiVersion":"admission.k8s.io/v1","kind":"AdmissionReview","response":{"uid":'
                else:
                    resp = {"uid": uid, "allowed": rec.mode == "allow"}
                    if rec.mode == "deny":
                        resp["status"] = {"code": 403, "message": "not on this shift"}
                    body = json.dumps({"apiVersion": "admission.k8s.io/v1", "kind": "AdmissionReview",
                                       "response": resp}).encode()
                self.send_response(200)
                self.send_header("Content-Type", "application/json")
                self.send_header("Content-Length", str(len(body)))
                self.end_headers()
                self.wfile.write(body)

            def log_message(self, *a):
                pass

        self.httpd = http.server.ThreadingHTTPServer(("127.0.0.1", 0), Handler)
        ctx = ssl.SSLContext(ssl.PROTOCOL_TLS_SERVER)
        ctx.load_cert_chain(os.path.join(cert_dir, "tls.crt"), os.path.join(cert_dir, "tls.key"))
        self.httpd.socket = ctx.wrap_socket(self.httpd.socket, server_side=True)
        self.port = self.httpd.server_address[1]
        self.thread = threading.Thread(target=self.httpd.serve_forever, daemon=True)
        self.thread.start()

    def last(self, operation, name):
        return [r for r in self.requests if r["operation"] == operation and r["name"] == name][-1]

    def stop(self):
        self.httpd.shutdown()
        self.httpd.server_close()


@pytest.fixture(scope="module")
def certs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("hook-cert"))
    subprocess.run([binary("bgc-certgen"), d, "record-hook", "localhost", "127.0.0.1"], check=True, timeout=60)
    return d


def stack(certs, apiserver_args):
    rec = Recorder(certs)
    cl = Cluster(admission=False, controller=False, apiserver_args=apiserver_args).start()
    cl.admin.create("mutatingwebhookconfigurations", {
        "apiVersion": "admissionregistration.k8s.io/v1", "kind": "MutatingWebhookConfiguration",
        "metadata": {"name": "recorder"},
        "webhooks": [{"name": HOOK,
                      "rules": [{"apiGroups": ["bacchus.io"], "apiVersions": ["v1"],
                                 "resources": ["userbootstraps", "userbootstraps/status"], "scope": "*", "operations": ["CREATE", "UPDATE", "DELETE"]}],
                      "clientConfig": {"url": f"https://127.0.0.1:{rec.port}/mutate",
                                       "caBundle": open(os.path.join(certs, "caBundle.b64")).read().strip()},
                      "timeoutSeconds": 5, "sideEffects": "None", "admissionReviewVersions": ["v1"],
                      "failurePolicy": "Fail"}]})
    return cl, rec


@pytest.fixture(scope="module", params=["line-held", "history-compacted"])
def hooked(request, certs):
    """kube-lite with the recording webhook; `churn(c)` makes the history forget the commits
    before it: nothing when the history is long, five writes of the type when it holds four."""
    compacted = request.param == "history-compacted"
    cl, rec = stack(certs, ["--history", "4"] if compacted else [])
    n = [0]

    def churn():
        if compacted:
            for _ in range(5):
                n[0] += 1
                cl.admin.create("userbootstraps", ub(f"other-{n[0]}"))

    try:
        yield cl, rec, churn
    finally:
        cl.stop()
        rec.stop()


def ub(name, username=None):
    return {"apiVersion": "bacchus.io/v1", "kind": "UserBootstrap", "metadata": {"name": name, "labels": {"team": "a"}},
            "spec": {"kube_username": username or name}}


def before_commit(obj):
    meta = {k: v for k, v in obj["metadata"].items() if k not in AFTER_ADMISSION}
    return dict(obj, metadata=meta)


def test_review_objects_are_the_stored_and_the_written_object(hooked):
    c, rec, churn = hooked
    created = c.admin.create("userbootstraps", ub("alice"), field_manager="creator")
    req = rec.last("CREATE", "alice")
    assert req["oldObject"] is None
    assert before_commit(req["object"]) == before_commit(created)
    assert req["kind"] == {"group": "bacchus.io", "version": "v1", "kind": "UserBootstrap"}
    assert req["resource"] == req["requestResource"] == {"group": "bacchus.io", "version": "v1", "resource": "userbootstraps"}
    assert req["requestKind"] == req["kind"] and req["options"] == {"kind": "CreateOptions", "apiVersion": "meta.k8s.io/v1"}
    assert "namespace" not in req and "subResource" not in req and req["dryRun"] is False

    churn()
    got = c.admin.get("userbootstraps", "alice")
    assert got["metadata"]["managedFields"] and got["metadata"]["resourceVersion"] == created["metadata"]["resourceVersion"]
    updated = c.admin.merge_patch("userbootstraps", "alice", {"spec": {"kube_username": "alice2"}}, field_manager="patcher")
    req = rec.last("UPDATE", "alice")
    assert req["oldObject"] == got
    assert before_commit(req["object"]) == before_commit(updated)
    assert updated["metadata"]["generation"] == 2 and updated["spec"]["kube_username"] == "alice2"
    assert req["options"] == {"kind": "UpdateOptions", "apiVersion": "meta.k8s.io/v1"}

    # a status write: the subresource is named, oldObject is again the stored object
    churn()
    got = c.admin.get("userbootstraps", "alice")
    assert got == updated
    c.admin.merge_patch("userbootstraps", "alice", {"status": {"synchronized_with_sheet": True}}, sub="status")
    req = rec.last("UPDATE", "alice")
    assert req["oldObject"] == got and req["subResource"] == req["requestSubResource"] == "status"

    churn()
    got = c.admin.get("userbootstraps", "alice")
    assert got["status"] == {"synchronized_with_sheet": True}
    c.admin.delete("userbootstraps", "alice")
    req = rec.last("DELETE", "alice")
    assert req["oldObject"] == got and req["object"] is None
    assert req["options"] == {"kind": "DeleteOptions", "apiVersion": "meta.k8s.io/v1"}
    assert c.admin.get_or_none("userbootstraps", "alice") is None


def test_denied_and_malformed_responses_keep_their_status(hooked):
    """The texts are kube-lite's from before the request was built from cached and reused text."""
    c, rec, _ = hooked
    c.admin.create("userbootstraps", ub("bob"))
    try:
        rec.mode = "deny"
        for write in (lambda: c.admin.create("userbootstraps", ub("carol")),
                      lambda: c.admin.merge_patch("userbootstraps", "bob", {"spec": {"kube_username": "b2"}}),
                      lambda: c.admin.delete("userbootstraps", "bob")):
            with pytest.raises(ApiError) as e:
                write()
            assert e.value.code == 403 and e.value.reason == "Forbidden"
            assert e.value.message == f'admission webhook "{HOOK}" denied the request: not on this shift'
        rec.mode = "malformed"
        with pytest.raises(ApiError) as e:
            c.admin.merge_patch("userbootstraps", "bob", {"spec": {"kube_username": "b3"}})
        assert e.value.code == 500 and e.value.reason == "InternalError"
        assert e.value.message == (f'Internal error occurred: failed calling webhook "{HOOK}": failed to parse webhook '
                                   "response: EOF while parsing a value at line 1 column 80")
    finally:
        rec.mode = "allow"
    assert c.admin.get("userbootstraps", "bob")["spec"]["kube_username"] == "bob"
