"""The solve runs the schedule function the host test checked: after a real solve, ilqg_problem_last_schedule equals the
word ilqg_schedule_build returns for the same description, options, batch, mask and the device's CU count
(tests/test_schedule.py replays that function against the recorded schedules without a GPU)."""
import numpy as np
import pytest

import schedule_cases as sc
from ilqgames_amd import abi, hip

pytestmark = pytest.mark.gpu

OPTIONS = {"default": {}, "deterministic": {"deterministic": True}, "masked_3": {"masked": 3}}


@pytest.fixture(scope="module")
def num_cus():
    return hip.device_info()[1]


@pytest.mark.parametrize("dtype", [abi.F32, abi.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("scene", ["n14", "n24", "n4", "generic"])
def test_solve_runs_the_built_schedule(scene, dtype, num_cus):
    import torch
    spec = sc.make_spec(scene, 8)
    prob = hip.Problem(spec, dtype)
    for batch in (4, 5 * num_cus):
        bufs = prob.alloc_solve_buffers(batch)
        x0 = np.tile(np.asarray(spec.x0, dtype=np.float64), (batch, 1))
        for name, opts in OPTIONS.items():
            kw, active, mask = sc.solve_kwargs(opts), None, None
            if "masked" in opts:  # a free-running solve: it counts its mask and schedules for the instances taking part
                active = opts["masked"]
                mask = torch.zeros(batch, dtype=torch.int32, device="cuda")
                mask[:active] = 1
            else:
                kw["fixed_iters"] = 1
            for k in ("xs", "us", "P", "alpha"):
                bufs[k].zero_()
            prob.solve(x0, bufs, active=mask, **kw)
            torch.cuda.synchronize()
            want = hip.schedule_build(spec, dtype, batch, num_cus, active=active, **kw)["word"]
            assert prob.last_schedule() == want, (scene, batch, name, prob.last_schedule(), want)
