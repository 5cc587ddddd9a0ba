"""Pod networking (pkg/kubelet/network/kubenet, hostport, dockershim network set-up): with a
privileged rocshim every non-hostNetwork pod gets its own network/IPC/UTS namespaces wired by
the native `amdkube-bridge` CNI plugin (bridge + veth + host-local IPAM), so pods have their own
IPs, talk to each other across the bridge, keep namespaced sysctls to themselves, are reached
through held host ports, and leave nothing behind when deleted. Needs root (netlink, setns)."""
import asyncio
import os
import secrets
import socket
import subprocess

import pytest

from amdkube.localcluster import LocalCluster, wait_pod
from amdkube.runtime.images import NATIVE_BIN
from amdkube.runtime.network import KubenetNetwork
from tests.conftest import run

CNI_BIN = os.path.join(NATIVE_BIN, "cni")


def _netns_capable() -> bool:
    if not os.path.exists(os.path.join(CNI_BIN, "amdkube-bridge")):
        return False
    # an ordinary user gets a network namespace with the user namespace the test then runs in (needs_root)
    return os.geteuid() != 0 or subprocess.run(["unshare", "-n", "true"], capture_output=True).returncode == 0


needs_netns = pytest.mark.skipif(not _netns_capable(), reason="needs network namespaces and the built bridge plugin")

SERVER = ("import socket\n"
          "s = socket.socket(); s.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1); s.bind(('0.0.0.0', 8080)); s.listen(8)\n"
          "while True:\n"
          "    c, a = s.accept()\n"
          "    r = open('/proc/sys/net/ipv4/ip_local_port_range').read().split()\n"
          "    c.sendall(f'{socket.gethostname()} {r[0]}-{r[1]} {a[0]}'.encode()); c.close()\n")


def _ifaces():
    with open("/proc/net/dev") as f:
        return {ln.split(":")[0].strip() for ln in f.read().splitlines()[2:]}


async def _fetch(host, port, timeout=5.0):
    r, w = await asyncio.wait_for(asyncio.open_connection(host, port), timeout)
    data = await asyncio.wait_for(r.read(), timeout)
    w.close()
    return data.decode()


@needs_netns
@pytest.mark.needs_root(net=True)
def test_pod_namespaces_bridge_hostport_sysctl_and_teardown(tmp_path):
    bridge = "akb" + secrets.token_hex(4)
    subnet = f"10.{96 + secrets.randbelow(4)}.{secrets.randbelow(250)}.0/24"
    host_range = open("/proc/sys/net/ipv4/ip_local_port_range").read()
    before = _ifaces()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        host_port = s.getsockname()[1]

    async def go():
        net = KubenetNetwork([CNI_BIN], str(tmp_path / "net"), bridge=bridge, mtu=1400)
        net.set_pod_cidr(subnet)
        async with LocalCluster(gpus="none", relist_period=0.2, with_controllers=False,
                                shim_kw={"network": net, "pod_namespaces": True}) as lc:
            c = lc.client
            await c.create({"apiVersion": "v1", "kind": "Pod", "metadata": {
                "name": "srv", "annotations": {"security.alpha.kubernetes.io/sysctls": "net.ipv4.ip_local_port_range=20000 30000"}},
                "spec": {"hostname": "web", "containers": [{"name": "c", "image": "busybox", "command": ["python3", "-c", SERVER],
                                                            "ports": [{"containerPort": 8080, "hostPort": host_port}]}]}},
                           "default")
            srv = await wait_pod(c, "default", "srv", timeout=30)
            ip = srv["status"]["podIP"]
            assert ip and ip != lc.kubelet.cfg.node_ip and ip.rsplit(".", 1)[0] == subnet.rsplit(".", 1)[0], ip
            # reachable at its own address from the node (through the bridge) ...
            for _ in range(100):
                try:
                    out = await _fetch(ip, 8080)
                    break
                except OSError:
                    await asyncio.sleep(0.1)
            host, rng, peer = out.split()
            assert host == "web" and rng == "20000-30000" and peer == subnet.rsplit(".", 1)[0] + ".1"   # the gateway
            # ... through the held host port ...
            assert (await _fetch("127.0.0.1", host_port)).startswith("web 20000-30000")
            # ... and from another pod across the bridge, from the client pod's own address
            await c.create({"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "cli"}, "spec": {
                "restartPolicy": "Never", "containers": [{"name": "c", "image": "busybox", "command": [
                    "python3", "-c", f"import socket; s = socket.create_connection(('{ip}', 8080), 5); print(s.recv(200).decode())"]}]}},
                           "default")
            cli = await wait_pod(c, "default", "cli", ("Succeeded", "Failed"), timeout=30)
            assert cli["status"]["phase"] == "Succeeded", cli["status"]
            logs = await c.request("GET", "/api/v1/namespaces/default/pods/cli/log", raw=True)
            logs = logs.decode() if isinstance(logs, bytes) else logs
            assert logs.split()[0] == "web" and logs.split()[2] == cli["status"]["podIP"]
            # the host's own sysctl is untouched; a second pod gets its own veth
            assert open("/proc/sys/net/ipv4/ip_local_port_range").read() == host_range
            during = _ifaces()
            assert bridge in during and len([i for i in during - before if i.startswith("veth")]) >= 1
            # deleting the pods removes their veths and releases their addresses
            for name in ("srv", "cli"):
                await c.delete("pods", name, "default", grace=0)
            for _ in range(200):
                if not [i for i in _ifaces() - before if i.startswith("veth")]:
                    break
                await asyncio.sleep(0.1)
            assert not [i for i in _ifaces() - before if i.startswith("veth")]
            ipam = tmp_path / "net" / "ipam" / "kubenet"
            assert not [f for f in os.listdir(ipam) if f[0].isdigit()]
            # the host port is free again (no listener; TIME_WAIT leftovers of the fetches are fine)
            with socket.socket() as s2:
                s2.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
                s2.bind(("0.0.0.0", host_port))
                s2.listen(1)
    try:
        run(go(), 120)
    finally:
        subprocess.run([os.path.join(CNI_BIN, "amdkube-bridge"), "--delete-bridge", bridge], capture_output=True)
    assert bridge not in _ifaces()


def test_sysctls_refused_without_pod_namespaces():
    async def go():
        async with LocalCluster(gpus="none", relist_period=0.2, with_controllers=False) as lc:
            c = lc.client
            await c.create({"apiVersion": "v1", "kind": "Pod", "metadata": {
                "name": "sy", "annotations": {"security.alpha.kubernetes.io/sysctls": "net.ipv4.tcp_syncookies=0"}},
                "spec": {"containers": [{"name": "c", "image": "busybox", "command": ["sleep", "5"]}]}}, "default")
            for _ in range(100):
                evs, _ = await c.list("events", "default")
                hit = [e for e in evs if e.get("reason") == "FailedCreatePodSandBox" and "refusing to change host kernel parameters" in e["message"]]
                if hit:
                    break
                await asyncio.sleep(0.1)
            assert hit
    run(go(), 60)
