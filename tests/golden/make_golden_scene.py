"""Generate tests/golden/scene_golden.npz: the REAL Utils.depth2xyzmap of the reference (Utils.py:239-251) on seeded depth images of
both dtypes, with values on both sides of the 0.1 validity threshold in each.  Build container only (`python
tests/golden/make_golden_scene.py`); the GPU box has no /root/reference and uses the committed file.

Utils.py imports packages that are not installable here; depth2xyzmap needs numpy alone, so the function's own source text is cut out
of the file and executed unmodified in a namespace that holds numpy."""
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

with open('/root/reference/Utils.py') as f:
    src = f.read()
m = re.search(r'^def depth2xyzmap\(.*?(?=^\S)', src, flags=re.S | re.M)
ns = {'np': np}
exec(compile(m.group(0), '/root/reference/Utils.py', 'exec'), ns)
depth2xyzmap = ns['depth2xyzmap']

K = np.array([[2257.75, 0, 40.3], [0, 2257.49, 30.7], [0, 0, 1]])
rng = np.random.default_rng(11)
d64 = rng.uniform(0.3, 1.2, (24, 20))
d64[0, :8] = [0.0, 0.05, 0.1, np.nextafter(0.1, 0), np.nextafter(0.1, 1), float(np.float32(0.1)), np.nextafter(float(np.float32(0.1)), 0), 0.0999]
d64[5, 3] = 2.9
d32 = d64.astype(np.float32)
f = np.float32(0.1)
d32[1, :4] = [f, np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(1)), np.float32(0.0999)]
np.savez_compressed(os.path.join(HERE, 'scene_golden.npz'), K=K, depth_f64=d64, depth_f32=d32, xyz_f64=depth2xyzmap(d64, K),
                    xyz_f32=depth2xyzmap(d32, K))
print('written', os.path.join(HERE, 'scene_golden.npz'))
