"""Per-instance routes, the checks that need no GPU: the prototypes of the C header, what ilqg_instance_routes_check
accepts and refuses (host only: the library is loaded without a device, as tests/test_instance_params.py does), the C++
mirror's resolution of AddRoute(object) / AddRoute(index) to polylines of the descriptor, and the one segment function
the host builder and the device kernel share, called from a sanitised stand-alone program on every scene's polylines."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from ilqgames_amd import abi, examples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    from ilqgames_amd import hip as h
    if not os.path.exists(h.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return h


def test_c_header_declares_the_calls_and_keeps_abi_version_9():
    """The snippet takes the address of every function with its exact prototype: a missing or differently typed
    declaration does not compile (-Werror)."""
    src = r'''
#include <stdio.h>
#include "ilqg.h"
typedef ilqg_status (*declare_fn)(ilqg_problem*, int32_t, const int32_t*);
typedef ilqg_status (*bind_fn)(ilqg_problem*, int32_t, const float*, void*);
typedef ilqg_status (*check_fn)(const ilqg_problem_desc*, int32_t, const int32_t*);
typedef ilqg_status (*table_fn)(const ilqg_problem_desc*, int32_t, void*, int32_t, int32_t*);
int main(void) {
  declare_fn d = &ilqg_problem_declare_instance_routes;
  bind_fn b = &ilqg_problem_bind_instance_routes;
  check_fn c = &ilqg_instance_routes_check;
  table_fn t = &ilqg_segment_table_build;
  (void)d; (void)b; (void)c; (void)t;
  printf("%d\n", (int)ILQG_ABI_VERSION);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", c, "-o", exe + ".o"])
    assert abi.ABI_VERSION == 9


def test_library_exports_the_calls(hip):
    for name in ("ilqg_problem_declare_instance_routes", "ilqg_problem_bind_instance_routes", "ilqg_instance_routes_check",
                 "ilqg_segment_table_build"):
        assert name in hip.EXPORTS and hasattr(hip.lib(), name), name
    assert hip.lib().ilqg_abi_version() == 9


ACCEPTED = [
    (examples.modified_three_player_intersection, [1, 0, 2]),
    (examples.cost_zoo_scene, [2, 1]),
    (examples.two_player_reachability, [0]),
    (examples.one_player_reachability, [0]),
    (examples.mixed_dubins_car_scene, [0]),
    (examples.roundabout_merging, [0, 3]),
]


@pytest.mark.parametrize("make,polylines", ACCEPTED)
def test_check_accepts(hip, make, polylines):
    spec = make()
    assert max(polylines) < len(spec.polylines)
    hip.instance_routes_check(spec, polylines)
    hip.instance_routes_check(spec, list(reversed(polylines)))  # a row holds them in the caller's order
    for q in polylines:
        hip.instance_routes_check(spec, [q])
    hip.instance_routes_check(spec, [])


def _refused(hip, spec, polylines, polyline, *words):
    with pytest.raises(hip.IlqgError) as e:
        hip.instance_routes_check(spec, polylines)
    assert e.value.status == abi.ERR_UNSUPPORTED, str(e.value)
    msg = str(e.value)
    assert "polyline %d" % polyline in msg, msg
    for w in words:
        assert w in msg, msg


def test_check_refuses_with_a_message_naming_the_polyline(hip):
    s = examples.modified_three_player_intersection()
    n = len(s.polylines)
    _refused(hip, s, [-1], -1, "out of range")
    _refused(hip, s, [n], n, "out of range")
    _refused(hip, s, [1, n], n, "out of range")  # one refused polyline refuses the declaration
    _refused(hip, s, [0, 1, 0], 0, "twice")
    with pytest.raises(hip.IlqgError) as e:
        hip._check(hip.lib().ilqg_instance_routes_check(None, 0, None))
    assert e.value.status == abi.ERR_INVALID
    # a scene without polylines has none to declare
    u = examples.two_player_unicycle_4d_scene()
    assert len(u.polylines) == 0
    _refused(hip, u, [0], 0, "out of range")
    hip.instance_routes_check(u, [])


def test_check_refuses_the_polyline_of_a_route_progress_term_and_names_the_term(hip):
    """ilqg_problem_create tabulates a ROUTE_PROGRESS term's per-step nominals from the baked polyline; a polyline no such
    term refers to stays accepted in the same problem, also when a lane cost shares the refused one."""
    s = examples.modified_three_player_intersection()
    term = s.route_progress(0, 5.0, 4.0, 0, (0, 1), 10.0)
    assert s.terms[term]["kind"] == abi.COST_ROUTE_PROGRESS and s.terms[term]["polyline"] == 0
    _refused(hip, s, [0], 0, "term %d" % term, "ROUTE_PROGRESS")
    _refused(hip, s, [1, 0], 0, "term %d" % term, "ROUTE_PROGRESS")
    hip.instance_routes_check(s, [1])
    hip.instance_routes_check(s, [2, 1])
    # NOMINAL_PATH_LENGTH is time-dependent too but reads no polyline: nothing is refused on its account
    s2 = examples.modified_three_player_intersection()
    s2.nominal_path_length(0, 5.0, 1, 4.0)
    hip.instance_routes_check(s2, [0, 1, 2])


def test_declare_and_bind_without_a_handle_return_what_the_neighbouring_calls_return(hip):
    """No handle exists without a device; on a null handle the declare and bind calls answer as
    ilqg_problem_declare_instance_params / ilqg_problem_bind_instance_values do."""
    lib = hip.lib()
    arr = (hip.C.c_int32 * 1)(0)
    neighbours = (lib.ilqg_problem_declare_instance_subsystem_params(None, 1, arr),
                  lib.ilqg_problem_bind_instance_values(None, 1, None))
    assert lib.ilqg_problem_declare_instance_routes(None, 1, arr) == neighbours[0] == abi.ERR_INVALID
    assert lib.ilqg_problem_bind_instance_routes(None, 1, None, None) == neighbours[1] == abi.ERR_INVALID


def _demo():
    import __graft_entry__
    exe = os.path.join(ROOT, "tests", "host", "_bin", "instance_routes_demo")
    if not os.path.exists(exe):
        __graft_entry__.build_host()
    return exe


def test_cpp_mirror_resolves_routes_by_address_and_by_index_to_the_same_declaration():
    """tests/host/instance_routes_demo.cpp resolve: the headline scene built with the mirrored classes; AddRoute(&lane2)
    and AddRoute(1) -> polyline 1, a polyline of no cost -> false with a reason, AddRoute(3) -> false, the same polyline
    twice -> refused by the library, routes named to a caller that takes none -> false; the description it flattens is
    the builder's."""
    lines = subprocess.check_output([_demo(), "resolve"], text=True, timeout=120).splitlines()
    assert lines[0] == "address 1" and lines[1] == "index 1"
    foreign = lines[2].split(None, 2)
    assert foreign[:2] == ["foreign", "0"] and "no polyline of the problem" in foreign[2]
    p3 = lines[3].split(None, 2)
    assert p3[:2] == ["polyline3", "0"] and "polyline 3" in p3[2]
    twice = lines[4].split(None, 2)
    assert twice[0] == "twice" and int(twice[1]) == abi.ERR_UNSUPPORTED and "polyline 1" in twice[2] and "twice" in twice[2]
    none = lines[5].split(None, 2)
    assert none[:2] == ["noroutes", "0"] and "routes" in none[2]
    assert lines[6] == "dump"
    dump = abi.ProblemSpec.from_dump("\n".join(lines[7:]))
    s = examples.modified_three_player_intersection()
    assert dump.canonical() == s.canonical()
    assert [tuple(p) for p in dump.polylines[1]] == [tuple(p) for p in s.polylines[1]]


SEGMENT_PROGRAM = r'''
// Reads [count | per polyline: npts, points (float) | nf, float table | nd, double table] and rebuilds both tables with
// the segment function the library's host builder and its device kernel share; prints the number of differing bytes.
#include <cstdio>
#include <cstring>
#include <vector>
#include "ilqg_segment.hpp"

template <class S>
static long long differing(const std::vector<std::vector<float>>& polys, const std::vector<S>& want) {
  std::vector<S> got;
  for (const auto& pts : polys) {
    const int nseg = int(pts.size() / 2) - 1;
    for (int c = 0; c < nseg; c++) {
      S sg[3 * ilqg::kSegmentScalars];
      ilqg::segment_and_shortcuts(pts.data(), nseg, c, sg);
      got.insert(got.end(), sg, sg + 3 * ilqg::kSegmentScalars);
    }
  }
  if (got.size() != want.size()) return -1;
  long long bad = 0;
  const unsigned char* a = reinterpret_cast<const unsigned char*>(got.data());
  const unsigned char* b = reinterpret_cast<const unsigned char*>(want.data());
  for (size_t i = 0; i < got.size() * sizeof(S); i++) bad += a[i] != b[i];
  return bad;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  auto rd = [&](void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; };
  int count = 0;
  if (!rd(&count, sizeof(int))) return 3;
  std::vector<std::vector<float>> polys(count);
  for (auto& p : polys) {
    int npts = 0;
    if (!rd(&npts, sizeof(int))) return 3;
    p.resize(2 * size_t(npts));
    if (!rd(p.data(), sizeof(float) * p.size())) return 3;
  }
  int nf = 0, nd = 0;
  if (!rd(&nf, sizeof(int))) return 3;
  std::vector<float> tf(nf);
  if (!rd(tf.data(), sizeof(float) * tf.size())) return 3;
  if (!rd(&nd, sizeof(int))) return 3;
  std::vector<double> td(nd);
  if (!rd(td.data(), sizeof(double) * td.size())) return 3;
  std::fclose(f);
  std::printf("%lld %lld %d\n", differing<float>(polys, tf), differing<double>(polys, td), nf);
  return 0;
}
'''


def test_shared_segment_function_rebuilds_every_scene_table_bytewise_under_sanitizers(hip):
    """A stand-alone program with its own main, compiled with -fsanitize=address,undefined against
    ilqgames_amd/csrc/ilqg_segment.hpp alone, rebuilds the segment tables of every scene (and of one with a zero-length
    segment) from their polylines; the tables it is compared with are build_segments' (ilqg_segment_table_build, called
    here from the unsanitised library).  Nothing sanitised is loaded into Python."""
    scenes = [make() for make in examples.CONFIGS.values()]
    scenes += [examples.cost_zoo_scene(), examples.mixed_dubins_car_scene(), examples.two_player_reachability(),
               examples.one_player_reachability()]
    degenerate = examples.modified_three_player_intersection()
    degenerate.polylines[1][3] = degenerate.polylines[1][2]  # a zero-length segment: NaN directions, the same bits
    scenes.append(degenerate)
    scenes = [s for s in scenes if s.polylines]
    assert len(scenes) >= 8
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "segments.cpp")
        open(src, "w").write(SEGMENT_PROGRAM)
        exe = os.path.join(td, "segments")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-ffp-contract=off", "-I", os.path.join(ROOT, "ilqgames_amd", "csrc"), src, "-o", exe])
        total = 0
        for k, spec in enumerate(scenes):
            tf, tdbl = hip.segment_table(spec, abi.F32), hip.segment_table(spec, abi.F64)
            assert tf.shape == tdbl.shape == (sum(len(p) - 1 for p in spec.polylines), 21)
            path = os.path.join(td, "scene%d.bin" % k)
            with open(path, "wb") as f:
                f.write(np.int32(len(spec.polylines)).tobytes())
                for p in spec.polylines:
                    f.write(np.int32(len(p)).tobytes())
                    f.write(np.asarray(p, dtype=np.float32).tobytes())
                f.write(np.int32(tf.size).tobytes() + tf.tobytes())
                f.write(np.int32(tdbl.size).tobytes() + tdbl.tobytes())
            out = subprocess.run([exe, path], check=True, text=True, capture_output=True, timeout=60)
            assert out.stderr == "", out.stderr
            bad_f, bad_d, nf = (int(v) for v in out.stdout.split())
            assert (bad_f, bad_d, nf) == (0, 0, tf.size), (k, out.stdout)
            total += nf
        assert total > 0
    assert np.isnan(hip.segment_table(degenerate, abi.F32)[3, 5])
