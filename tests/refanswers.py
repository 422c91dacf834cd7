"""The unmodified reference's answers, stored with the suite (tests/golden/refanswers/<test module>.json).

A test that pins something to the reference asks `refans.take(fn)` for each answer, `fn` being the reference call.
Where the reference tree is present (oracle/ref_loader.py) `fn` runs and its value is held to the stored one, so the
stored answers cannot drift from what the reference says; NHD_RECORD_REFERENCE=1 rewrites them instead.  Everywhere
else the stored answers stand in for the reference, in the order the test asked for them, on the same seeded inputs
built from the stand-ins (workload/refmodel.py) - a test with no stored answers fails, it does not skip.

Values keep their Python types through JSON: tuples, dicts with non-string keys and byte strings are tagged."""
import json
import os

from oracle import ref_loader

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refanswers")
RECORD = os.environ.get("NHD_RECORD_REFERENCE") == "1"
_files = {}


def encode(v):
    if isinstance(v, tuple):
        return {"t": [encode(x) for x in v]}
    if isinstance(v, list):
        return [encode(x) for x in v]
    if isinstance(v, dict):
        return {"d": [[encode(k), encode(x)] for k, x in v.items()]}
    if isinstance(v, (bytes, bytearray)):
        return {"b": bytes(v).hex()}
    if hasattr(v, "item") and not hasattr(v, "__len__"):     # numpy scalars
        return v.item()
    assert v is None or isinstance(v, (bool, int, float, str)), type(v)
    return v


def decode(v):
    if isinstance(v, list):
        return [decode(x) for x in v]
    if isinstance(v, dict):
        (tag, x), = v.items()
        if tag == "t":
            return tuple(decode(y) for y in x)
        if tag == "d":
            return {decode(k): decode(y) for k, y in x}
        return bytes.fromhex(x)
    return v


def _path(module):
    return os.path.join(GOLDEN, module + ".json")


def _load(module):
    if module not in _files:
        p = _path(module)
        _files[module] = json.load(open(p)) if os.path.exists(p) else {}
    return _files[module]


def save(module):
    os.makedirs(GOLDEN, exist_ok=True)
    data = _files[module]
    with open(_path(module), "w") as f:
        json.dump({k: data[k] for k in sorted(data)}, f, separators=(",", ":"))
        f.write("\n")


class Answers:
    def __init__(self, module, test):
        self.module, self.test = module, test
        self.live = ref_loader.available()
        self.ref = ref_loader.load() if self.live else None      # the reference's classes, or None: build stand-ins
        stored = _load(module).get(test)
        if not self.live and stored is None:
            raise AssertionError(f"no stored reference answers for {module}::{test} (record them where the reference is "
                                 f"present: NHD_RECORD_REFERENCE=1 pytest {module.replace('.', '/')}.py)")
        self.stored = [] if stored is None else stored
        self.out = []

    def take(self, fn):
        """The reference's answer: fn() where the reference is present (held to the stored one), the stored one elsewhere."""
        k = len(self.out)
        if self.live:
            v = encode(fn())
            if not RECORD:
                assert k < len(self.stored), f"{self.test}: answer {k} was never stored (NHD_RECORD_REFERENCE=1 to record)"
                assert v == self.stored[k], f"{self.test}: the reference's answer {k} differs from the stored one"
        else:
            assert k < len(self.stored), f"{self.test}: asks for answer {k}, {len(self.stored)} stored"
            v = self.stored[k]
        self.out.append(v)
        return decode(v)

    def finish(self):
        if self.live and RECORD:
            _load(self.module)[self.test] = self.out
            save(self.module)
        else:
            assert len(self.out) == len(self.stored), f"{self.test}: {len(self.out)} answers taken, {len(self.stored)} stored"
