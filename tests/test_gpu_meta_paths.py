"""Which way the baidu_std metas go when plain calls and calls with an HBM
attachment share one connection (policy/baidu_std_meta.h): a plain 32 B echo
and an echo with a 4 KiB device attachment alternate, eight of each. The
attachment's bytes come back right, the device calls, whose metas carry
device payload descriptors, take the generic path both ways, and the plain
calls take the fast one on all four legs, because the first device call has
had the hellos of the connection answered."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LEGS = ("request_packed", "request_parsed", "response_packed", "response_parsed")


def _counts(native):
    v = native.dump_vars("baidu_std_meta_*")
    return {k[len("baidu_std_meta_"):]: int(x) for k, x in v.items()}


def test_plain_and_device_calls_alternate_on_one_connection():
    from brpc_amd import native
    from brpc_amd.models import start_echo_server
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    s = start_echo_server("127.0.0.1:0", gpu_device=0)
    try:
        # Channels share a connection when they would talk the same way, and
        # asking for the device transport is part of that: the plain press
        # asks for it too (it has no attachment to lend), so both presses
        # reach the server over one connection. check_echo compares each
        # echoed message and attachment on the host.
        device = native.Press({"server": s.address, "concurrency": 1, "request_size": 32, "attachment_size": 4096,
                               "device_attachment": True, "gpu_device": 0, "check_echo": True})
        plain = native.Press({"server": s.address, "concurrency": 1, "request_size": 32, "device_attachment": True,
                              "gpu_device": 0, "check_echo": True})
        c0, x0 = _counts(native), native.gpu.xgmi_stats()
        for _ in range(8):
            device.run_requests(1)
            plain.run_requests(1)
        c1, x1 = _counts(native), native.gpu.xgmi_stats()
        ds, ps = device.stats(), plain.stats()
    finally:
        s.stop()
    assert ds["error"] == 0 and ds["success"] == 8, ds
    assert ps["error"] == 0 and ps["success"] == 8, ps
    delta = {k: c1[k] - c0[k] for k in c1}
    print("meta paths:", delta, "payloads lent:", x1["sent_payloads"] - x0["sent_payloads"])
    # device attachments went out as descriptors (the first request, which
    # carries the hellos, has no transport yet and is staged inline)
    assert x1["sent_payloads"] - x0["sent_payloads"] > 0
    for leg in LEGS:
        assert delta[leg + "_generic"] == 8, (leg, delta)
        assert delta[leg + "_fast"] == 8, (leg, delta)
