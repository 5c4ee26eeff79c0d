"""Winners of the convolution autotuner (drba_amd.ops._tune), kept across processes.

One JSON file per *identity*: the ABI version, a SHA-256 of the bytes of the loaded libdrba_hip.so, the device name, its
gcnArchName and its CU count.  A winner measured on other kernels or on another device is never offered.  An entry maps
(kind, shape tuple, sorted family set) -- the key _tune uses -- to the winning configuration id with the winner's and
the runner-up's best readings in microseconds, or records that no configuration accepts the shape.

    {"format": 1, "identity": {...}, "entries": {"[\"conv3x3\", [1, 39, 192, 8, 12, 2], [0, 1, 2, 3, 4]]":
        {"cfg": 7, "best_us": 41.3, "runner_up_us": 42.0}, "[\"conv3x3_shuffle\", ...]": {"none": true}}}

The file is input from outside the program: whatever in it is malformed is ignored (never an exception) and overwritten
by the next store.  Writes merge with what is on disk under an advisory lock and go through a temporary file and
os.replace, so concurrent writers (the ranks of a sharded run, unrelated processes) lose no entries; a store is
written through on every new winner.

DRBA_TUNE_CACHE is the only switch: a directory, `1` (${XDG_CACHE_HOME:-~/.cache}/drba_amd) or `0` (off).  Unset means
off in the library and on in the command line (drba_amd.infer.main calls default_on()).
"""
import hashlib
import json
import os
import tempfile
import warnings

try:
    import fcntl
except ImportError:  # no advisory locks on this platform: the replace is still atomic, concurrent writers may lose entries
    fcntl = None

FORMAT = 1
MAX_CFG = 4096  # no kernel table comes near it: an id beyond it is a damaged file
ENV = "DRBA_TUNE_CACHE"
_PREFIX, _SUFFIX = "tune-", ".json"
_IDENTITY_KEYS = ("abi", "lib_sha256", "device", "arch", "cus")

_default_on = False
_stores = {}
_lib_sha = {}


def default_on(on=True):
    """What an unset DRBA_TUNE_CACHE means from now on in this process (the command line: on)."""
    global _default_on
    _default_on = bool(on)


def default_dir():
    base = os.environ.get("XDG_CACHE_HOME") or os.path.join(os.path.expanduser("~"), ".cache")
    return os.path.join(base, "drba_amd")


def directory():
    """The directory DRBA_TUNE_CACHE selects, or None when the store is off."""
    v = os.environ.get(ENV)
    if v is None or v == "":
        return default_dir() if _default_on else None
    if v == "0":
        return None
    if v == "1":
        return default_dir()
    return v


def lib_sha256(path):
    st = os.stat(path)
    k = (path, st.st_size, st.st_mtime_ns)
    if k not in _lib_sha:
        h = hashlib.sha256()
        with open(path, "rb") as f:
            for block in iter(lambda: f.read(1 << 20), b""):
                h.update(block)
        _lib_sha[k] = h.hexdigest()
    return _lib_sha[k]


def device_identity(index=None):
    """The identity of this process on the current (or given) device.  Needs the built library and a GPU."""
    import torch

    from drba_amd import _lib
    _lib.load()
    index = torch.cuda.current_device() if index is None else index
    p = torch.cuda.get_device_properties(index)
    return make_identity(_lib.ABI_VERSION, lib_sha256(_lib.LIB_PATH), p.name, getattr(p, "gcnArchName", ""),
                         p.multi_processor_count)


def make_identity(abi, lib_sha, device, arch, cus):
    return {"abi": int(abi), "lib_sha256": str(lib_sha), "device": str(device), "arch": str(arch), "cus": int(cus)}


# tests (and anything else without a device) replace this: a callable (device index or None) -> the identity dict
identity_provider = device_identity


def identity_digest(identity):
    return hashlib.sha256(json.dumps(identity, sort_keys=True).encode()).hexdigest()[:20]


def file_name(identity):
    return _PREFIX + identity_digest(identity) + _SUFFIX


def encode_key(shape_key, families):
    """(kind, ints...) + the sorted family tuple -> the entry's name in the file, or None for a key that is not one of _tune's."""
    if not (isinstance(shape_key, tuple) and shape_key and isinstance(shape_key[0], str)):
        return None
    dims = shape_key[1:]
    if not all(isinstance(d, int) and not isinstance(d, bool) for d in dims):
        return None
    return json.dumps([shape_key[0], list(dims), sorted(int(f) for f in families)])


def _is_num(x):
    return isinstance(x, (int, float)) and not isinstance(x, bool) and x == x and abs(x) != float("inf")


def _valid_entry(e):
    if not isinstance(e, dict):
        return None
    if e.get("none") is True:
        return {"none": True}
    cfg = e.get("cfg")
    if not isinstance(cfg, int) or isinstance(cfg, bool) or not 0 <= cfg < MAX_CFG:
        return None
    out = {"cfg": cfg}
    for k in ("best_us", "runner_up_us"):
        v = e.get(k)
        out[k] = float(v) if _is_num(v) and v >= 0 else None
    return out


def _valid_identity(d):
    return (isinstance(d, dict) and set(d) == set(_IDENTITY_KEYS) and all(isinstance(d[k], int) and not isinstance(d[k], bool)
                                                                          for k in ("abi", "cus"))
            and all(isinstance(d[k], str) for k in ("lib_sha256", "device", "arch")))


def read_file(path, identity=None):
    """-> (identity block, {entry name: entry}) of a store file; (None, {}) for anything that is not one.  With `identity`
    the block must equal it.  Entries that are malformed are dropped one by one.  Never raises."""
    try:
        with open(path, "r", encoding="utf-8") as f:
            d = json.load(f)
        if not isinstance(d, dict) or d.get("format") != FORMAT or not _valid_identity(d.get("identity")):
            return None, {}
        if identity is not None and d["identity"] != identity:
            return None, {}
        if os.path.basename(path) != file_name(d["identity"]):  # a file copied over another identity's name
            return None, {}
        raw = d.get("entries")
        if not isinstance(raw, dict):
            return d["identity"], {}
        out = {}
        for k, e in raw.items():
            v = _valid_entry(e)
            if v is not None and _valid_name(k):
                out[k] = v
        return d["identity"], out
    except (OSError, ValueError, TypeError, RecursionError, UnicodeError):
        return None, {}


def _valid_name(k):
    try:
        d = json.loads(k)
    except (ValueError, TypeError, RecursionError):
        return False
    return (isinstance(d, list) and len(d) == 3 and isinstance(d[0], str) and isinstance(d[1], list) and isinstance(d[2], list)
            and all(isinstance(x, int) and not isinstance(x, bool) for x in d[1] + d[2]))


class _Lock:
    """Advisory lock on <file>.lock for the read-merge-replace of one store file."""

    def __init__(self, path):
        self.path, self.fd = path + ".lock", None

    def __enter__(self):
        if fcntl is None:
            return self
        self.fd = os.open(self.path, os.O_CREAT | os.O_RDWR, 0o644)
        try:
            fcntl.flock(self.fd, fcntl.LOCK_EX)
        except BaseException:
            os.close(self.fd)
            self.fd = None
            raise
        return self

    def __exit__(self, *exc):
        if self.fd is None:
            return
        try:
            fcntl.flock(self.fd, fcntl.LOCK_UN)
        finally:
            os.close(self.fd)
            self.fd = None


class Store:
    """The entries of one identity in one directory.  Nothing is created on disk before the first put."""

    def __init__(self, dirname, identity):
        self.dir, self.identity = dirname, dict(identity)
        self.path = os.path.join(dirname, file_name(self.identity))
        self._entries = None  # what the file held when first asked, plus what this process put
        self._mine = {}       # what this process put: written over whatever the file holds for the same names
        self._warned = False

    def _load(self):
        if self._entries is None:
            self._entries = read_file(self.path, self.identity)[1]
        return self._entries

    def __len__(self):
        return len(self._load())

    def entries(self):
        return dict(self._load())

    def get(self, shape_key, families):
        """-> None (unknown), {"none": True} or {"cfg": int, "best_us", "runner_up_us"}."""
        name = encode_key(shape_key, families)
        return None if name is None else self._load().get(name)

    def put(self, shape_key, families, cfg, best_us=None, runner_up_us=None):
        """Record a winner (cfg None: no configuration accepts the shape) and write the file through.  -> stored or not."""
        name = encode_key(shape_key, families)
        entry = _valid_entry({"none": True} if cfg is None else {"cfg": cfg, "best_us": best_us, "runner_up_us": runner_up_us})
        if name is None or entry is None:
            return False
        self._load()[name] = entry
        self._mine[name] = entry
        return self._flush()

    def _flush(self):
        try:
            os.makedirs(self.dir, exist_ok=True)
            with _Lock(self.path):
                merged = read_file(self.path, self.identity)[1]
                merged.update(self._mine)
                fd, tmp = tempfile.mkstemp(prefix=os.path.basename(self.path) + ".", suffix=".tmp", dir=self.dir)
                try:
                    with os.fdopen(fd, "w", encoding="utf-8") as f:
                        json.dump({"format": FORMAT, "identity": self.identity, "entries": merged}, f, sort_keys=True, indent=0)
                        f.flush()
                        os.fsync(f.fileno())
                    os.replace(tmp, self.path)
                except BaseException:
                    try:
                        os.unlink(tmp)
                    except OSError:
                        pass
                    raise
            for k, v in merged.items():  # what other writers added meanwhile is known from here on
                self._entries.setdefault(k, v)
            return True
        except OSError as e:
            if not self._warned:
                self._warned = True
                warnings.warn(f"drba_amd: the tuner's winners are not kept ({self.path}: {e}); this run is not affected")
            return False


def active(device=None):
    """The store of this process for the device of that index (None: the current one), or None when DRBA_TUNE_CACHE (or its
    default) says off."""
    d = directory()
    if d is None:
        return None
    ident = identity_provider(device)
    k = (os.path.abspath(d), identity_digest(ident))
    s = _stores.get(k)
    if s is None:
        s = _stores[k] = Store(d, ident)
    return s


def list_files(dirname):
    """[(path, identity, entries)] of every well-formed store file in the directory."""
    out = []
    try:
        names = sorted(os.listdir(dirname))
    except OSError:
        return out
    for n in names:
        if n.startswith(_PREFIX) and n.endswith(_SUFFIX):
            ident, ent = read_file(os.path.join(dirname, n))
            if ident is not None:
                out.append((os.path.join(dirname, n), ident, ent))
    return out


def clear(dirname):
    """Remove the files the store wrote in the directory (store files, their locks, left-over temporaries).  -> paths removed."""
    gone = []
    try:
        names = sorted(os.listdir(dirname))
    except OSError:
        return gone
    for n in names:
        if n.startswith(_PREFIX) and (n.endswith(_SUFFIX) or n.endswith(_SUFFIX + ".lock") or n.endswith(".tmp")):
            p = os.path.join(dirname, n)
            try:
                os.unlink(p)
                gone.append(p)
            except OSError:
                pass
    _stores.clear()
    return gone
