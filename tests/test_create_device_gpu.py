"""The device a create call picks (csrc/common.hpp: tbnav::pick_device, tbnav::DeviceGuard), for each of the five creates with the
smallest parameters its own case table uses: an index equal to the device count is TBNAV_ERR_INVALID_ARG and leaves no handle, -1 is
the calling thread's current device, 0 is device 0, and no call changes the thread's current device.  The current device is asked of
the HIP runtime the library itself runs on.  With more than one device the calls are also made with the last one current."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu


def _mppi(c, device):
    from cases import MPPI_BASE
    p = c.MppiParams()
    for k, v in MPPI_BASE.items():
        if isinstance(v, list):
            getattr(p, k)[:] = v
        else:
            setattr(p, k, v)
    p.device = device
    h = C.c_void_p()
    return c.lib().tbnav_mppi_create(C.byref(p), C.byref(h)), h


def _rbpf(c, device):
    from rtn_amd.rbpf import default_params
    p, h = default_params(N=2, k=4, device=device), C.c_void_p()
    return c.lib().tbnav_rbpf_create(C.byref(p), C.byref(h)), h


def _icp(c, device):
    from rtn_amd.icp import default_params
    p, h = default_params(device=device), C.c_void_p()
    return c.lib().tbnav_icp_create(C.byref(p), C.byref(h)), h


def _nav(c, device):
    p, h = c.NavParams(7, 5, 0.0, 0.0, 0.05, device, 0), C.c_void_p()
    return c.lib().tbnav_nav_create(C.byref(p), C.byref(h)), h


def _comm(c, device):
    uid, h = (C.c_uint8 * 128)(), C.c_void_p()
    assert c.lib().tbnav_comm_unique_id(C.cast(uid, C.c_void_p)) == c.OK
    return c.lib().tbnav_comm_create(C.cast(uid, C.c_void_p), 1, 0, device, C.byref(h)), h


CREATES = {"mppi": (_mppi, "tbnav_mppi_destroy"), "rbpf": (_rbpf, "tbnav_rbpf_destroy"), "icp": (_icp, "tbnav_icp_destroy"),
           "nav": (_nav, "tbnav_nav_destroy"), "comm": (_comm, "tbnav_comm_destroy")}


@pytest.fixture(scope="module")
def hip(gpu_pkg):
    """The HIP runtime mapped into this process (the one libtbnav_hip.so resolved its calls to)."""
    gpu_pkg.capi.lib()
    paths = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
    assert len(paths) == 1, paths
    rt = C.CDLL(paths.pop())
    rt.hipGetDevice.argtypes, rt.hipSetDevice.argtypes = [C.POINTER(C.c_int)], [C.c_int]
    return rt


def _current(hip):
    d = C.c_int(-7)
    assert hip.hipGetDevice(C.byref(d)) == 0
    return d.value


@pytest.mark.parametrize("name", sorted(CREATES))
def test_create_picks_its_device_and_leaves_the_current_one(gpu_pkg, hip, name):
    c = gpu_pkg.capi
    L = c.lib()
    create, destroy = CREATES[name]
    ndev = L.tbnav_device_count()
    before = _current(hip)
    try:
        for cur in sorted({0, ndev - 1}):
            assert hip.hipSetDevice(cur) == 0
            rc, h = create(c, ndev)
            assert rc == c.ERR_INVALID_ARG and not h.value, (name, cur, rc, h.value)
            assert _current(hip) == cur
            for device, lands_on in ((-1, cur), (0, 0)):
                rc, h = create(c, device)
                assert rc == c.OK and h.value, (name, cur, device, rc, L.tbnav_last_hip_error())
                if name == "comm":
                    assert L.tbnav_comm_device(h) == lands_on
                assert _current(hip) == cur, (name, cur, device)
                getattr(L, destroy)(h)
                assert _current(hip) == cur, (name, cur, device, "destroy")
    finally:
        hip.hipSetDevice(before)
