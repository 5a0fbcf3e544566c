"""Cases, references and a restatement of the scratch plan shared by tests/test_gpu_perm.py and
tests/test_perm_cpu.py: the device Fisher-Yates resolution and the global-minibatch member lists
(csrc/shuffle.hip), whose outputs are bit-identical to np.random.permutation.

* plan(n, count, room): csr_plan restated -- which layout (packed pairs / two arrays / the linked
  lists) and which geometry (partition size 2^logp, partitions, chunks) a call gets.  The CPU
  module ties it to the C++ through dppo_perm_resolve_scratch and asserts every geometry class
  below through it, so a case that drifts off its edge fails there, without a GPU.
* references: the sequential swap loop (adversarial targets), RandomState.permutation (random
  targets: the swap targets come from dppo_perm_targets_numpy on the same state) and
  global_lists, the member lists of one rank from whole permutations.

Test infrastructure only; NumPy and the host entry points, no GPU."""
import functools

import numpy as np

INF = 1 << 62
CHUNK = 32768          # kCsrChunk: steps per count / scatter workgroup
MAX_PARTS = 4096       # kCsrMaxParts
MIN_LOGP, MAX_LOGP = 11, 12
LDS_INTS = 16368       # csr_fill_index_kernel: (65536 - 64) / 4 ints of dynamic LDS
HEAP_ABOVE = 32        # csr_bucket_links heap-sorts a bucket of more steps than this
SEL_CHUNK = 16384      # kSelChunk: elements per shard_count / shard_write workgroup
FY_GRID = 8192 * 256   # fy_*_kernel: one element per thread up to here, grid-stride beyond


def _al(x):
    return (x + 63) // 64 * 64


def plan(n, count, room):
    """csr_plan(n, count, room): None where the linked lists run, else the layout and geometry
    {pack, logp, nparts, bpe, np, end, cap}; cap = the steps csr_fill_index_kernel holds in LDS."""
    if n < 2 or count < 1:
        return None
    logp = MIN_LOGP
    while logp < MAX_LOGP and ((n + (1 << logp) - 1) >> logp) > MAX_PARTS:
        logp += 1
    nparts = (n + (1 << logp) - 1) >> logp
    total = n * count
    if nparts > MAX_PARTS or total >= 0x7FFFFFFF:
        return None
    bpe = (n + CHUNK - 1) // CHUNK
    nprt = nparts * count
    geo = dict(logp=logp, nparts=nparts, bpe=bpe, np=nprt, cap=LDS_INTS - (2 << logp))
    tail = _al(count * bpe * nparts) + _al(nprt + 1)
    # packed: 8-B pairs | ent | dst | histograms | partition starts
    end = _al(2 * (total + 1)) + _al(total) + _al(total + count + 1) + tail
    if end <= room:
        return dict(geo, pack=True, end=end)
    # two arrays: step ids (then dst) | uint16 positions | ent | histograms | partition starts
    end = _al(total + count + 1) + _al((total + 1) // 2) + _al(total) + tail
    if end <= room:
        return dict(geo, pack=False, end=end)
    return None


def public_ints(n, count):
    return 3 * count * n


def packed_ints(n, count):
    """dppo_perm_resolve_scratch restated (test_perm_cpu.py asserts the equality)."""
    p = plan(n, count, INF)
    return max(p["end"], 3 * count * n) if p else 3 * count * n


# ---------------------------------------------------------------------------------------------
# resolution cases (n, count), each tagged with the class it is there for
# ---------------------------------------------------------------------------------------------
RESOLVE = [
    (1, 1, "tiny"), (2, 1, "tiny"), (3, 4, "tiny"), (17, 2, "tiny"),
    (362, 1, "fit-edge"), (363, 1, "fit-edge"), (533, 1, "fit-edge"), (534, 1, "fit-edge"),
    (2047, 1, "parts-1-2"), (2048, 1, "parts-1-2"), (2049, 3, "parts-1-2"),
    (32768, 1, "bpe-1-2"), (32769, 2, "bpe-1-2"),
    (294913, 1, "colscan-tail"),
    (2100001, 1, "basescan"), (524288, 4, "basescan"),
    (8388608, 1, "logp-edge"),
]
# n > 8,388,608: once per walk mode on the public and the packed scratch only
RESOLVE_BIG = [(8388609, 1, "logp-edge"), (16777216, 1, "logp-edge"), (16777217, 1, "big-lists")]

SCRATCH_KINDS = ("public", "packed", "packed-1")


def scratch_ints(n, count, kind):
    """The scratch size of `kind`, or None where it is no case of its own: below the public
    minimum (the entry point rejects it) or equal to the public size already run."""
    pub, pk = public_ints(n, count), packed_ints(n, count)
    if kind == "public":
        return pub
    v = pk if kind == "packed" else pk - 1
    return v if v > pub else None


def resolve_params(cases, kinds=SCRATCH_KINDS):
    return [(n, c, k) for n, c, _ in cases for k in kinds if scratch_ints(n, c, k) is not None]


def seed_of(n, count):
    return 3000 + 7 * n + count


@functools.lru_cache(maxsize=None)
def random_targets(n, count):
    """Swap targets [count * n] of the next `count` np.random permutations of RandomState(seed)."""
    from diamond import _native as N
    key, pos, _ = N.mt_state(np.random.RandomState(seed_of(n, count)))
    tg = np.empty(count * n, np.int32)
    N.perm_targets_numpy(key, pos, n, count, tg)
    tg.setflags(write=False)
    return tg


@functools.lru_cache(maxsize=None)
def random_reference(n, count):
    rs = np.random.RandomState(seed_of(n, count))
    ref = np.concatenate([rs.permutation(n) for _ in range(count)]).astype(np.int32)
    ref.setflags(write=False)
    return ref


# ---------------------------------------------------------------------------------------------
# adversarial but valid targets (every j_i <= i)
# ---------------------------------------------------------------------------------------------
ADVERSARIAL_KINDS = ("zeros", "identity", "shifted", "half", "mod64")
ADVERSARIAL_N = (12001, 20011)   # the value walk on `zeros` is O(n^2): n stays small
ADVERSARIAL_COUNT = 2


def adversarial_targets(kind, n):
    i = np.arange(n, dtype=np.int64)
    j = {"zeros": np.zeros(n, np.int64), "identity": i, "shifted": np.maximum(i - 1, 0),
         "half": i // 2, "mod64": i % 64}[kind]
    assert (j <= i).all() and (j >= 0).all()
    return j.astype(np.int32)


def fisher_yates(j):
    """a = arange(n); for i = n-1 .. 1: swap(a[i], a[j_i])"""
    a = list(range(len(j)))
    jl = [int(x) for x in j]
    for i in range(len(j) - 1, 0, -1):
        k = jl[i]
        a[i], a[k] = a[k], a[i]
    return np.asarray(a, np.int32)


@functools.lru_cache(maxsize=None)
def adversarial_reference(kind, n):
    ref = fisher_yates(adversarial_targets(kind, n))
    ref.setflags(write=False)
    return ref


# ---------------------------------------------------------------------------------------------
# what the kernels see of a target array (per epoch)
# ---------------------------------------------------------------------------------------------
def bucket_sizes(j):
    """Steps per bucket: bucket q = the steps i >= 1 with j_i = q."""
    return np.bincount(np.asarray(j[1:], np.int64), minlength=len(j))


def partition_sizes(j, logp):
    """Steps per partition of 2^logp positions (what csr_fill_index_kernel compares with cap)."""
    nparts = (len(j) + (1 << logp) - 1) >> logp
    return np.bincount(np.asarray(j[1:], np.int64) >> logp, minlength=nparts)


# ---------------------------------------------------------------------------------------------
# global-minibatch member lists
# ---------------------------------------------------------------------------------------------
# (T, Nl, world, M, E, ranks): Bg = T * Nl * world samples, Ng = Nl * world envs
LISTS = [
    (4, 2, 8, 8, 4, (0, 7)),        # Bg 64: ranks without members in some minibatches
    (3, 1, 2, 1, 1, (0, 1)),        # Bg 6, M = 1
    (5, 7, 3, 7, 3, (0, 1, 2)),     # Bg 105, Ng 21 (no power of two), mbg 15
    (2048, 1, 8, 16, 2, (5,)),      # exactly one chunk of 16,384, Nl = 1
    (16, 205, 5, 8, 2, (0, 2, 4)),  # Bg 16,400: a second chunk of 16 elements; mbg 2,050
    (64, 8200, 8, 5, 1, (3,)),      # Bg 4,198,400: 257 chunks
    # 257 chunks leave the `before` sum of shard_write_kernel at one round (chunk 256 adds 256
    # counts, one per thread); the second round starts with chunk 257:
    (64, 9601, 8, 4, 1, (6,)),      # Bg 4,915,712: 301 chunks, the last of 512 elements
]


def list_dims(case):
    T, Nl, world, M, E, _ = case
    Ng = Nl * world
    Bg = T * Ng
    return dict(T=T, Nl=Nl, world=world, M=M, E=E, Ng=Ng, Bg=Bg, B=T * Nl, mbg=Bg // M,
                chunks=(Bg + SEL_CHUNK - 1) // SEL_CHUNK)


def list_params():
    return [(k, r) for k, case in enumerate(LISTS) for r in case[5]]


def global_lists(perms, T, Nl, world, rank, M):
    """perms[E][Bg] (Bg = T * Nl * world, global flat index t * Ng + env) -> rank's
    local[E][T * Nl] (its members in permutation order, as t * Nl + env - env0) and seg[E][M + 1]
    (seg[e][j] = members among the first j * Bg / M entries of epoch e)."""
    perms = np.asarray(perms, np.int64)
    E, Bg = perms.shape
    Ng, env0, B = Nl * world, Nl * rank, T * Nl
    assert Bg == T * Ng and Bg % M == 0
    env = perms % Ng - env0
    keep = (env >= 0) & (env < Nl)
    loc = (perms // Ng) * Nl + env
    local = np.stack([loc[e][keep[e]] for e in range(E)]).astype(np.int32)
    assert local.shape == (E, B)
    kept = np.concatenate([np.zeros((E, 1), np.int64), np.cumsum(keep, axis=1)], axis=1)
    seg = kept[:, np.arange(M + 1) * (Bg // M)].astype(np.int32)
    assert (seg[:, M] == B).all()
    return local, seg


def global_lists_loop(perms, T, Nl, world, rank, M):
    """global_lists, sample by sample."""
    E, Bg = len(perms), len(perms[0])
    Ng, env0 = Nl * world, Nl * rank
    local, seg = [], []
    for e in range(E):
        row, marks = [], []
        for p in range(Bg):
            if p % (Bg // M) == 0:
                marks.append(len(row))
            t, env = divmod(int(perms[e][p]), Ng)
            if env0 <= env < env0 + Nl:
                row.append(t * Nl + env - env0)
        local.append(row)
        seg.append(marks + [len(row)])
    return np.asarray(local, np.int32).reshape(E, -1), np.asarray(seg, np.int32)


@functools.lru_cache(maxsize=None)
def list_inputs(k):
    """(targets [E * Bg], permutations [E][Bg]) of list case k, from one RandomState."""
    from diamond import _native as N
    d = list_dims(LISTS[k])
    key, pos, _ = N.mt_state(np.random.RandomState(5000 + k))
    tg = np.empty(d["E"] * d["Bg"], np.int32)
    N.perm_targets_numpy(key, pos, d["Bg"], d["E"], tg)
    rs = np.random.RandomState(5000 + k)
    perms = np.stack([rs.permutation(d["Bg"]) for _ in range(d["E"])]).astype(np.int32)
    tg.setflags(write=False)
    perms.setflags(write=False)
    return tg, perms


@functools.lru_cache(maxsize=None)
def list_reference(k, rank):
    d = list_dims(LISTS[k])
    local, seg = global_lists(list_inputs(k)[1], d["T"], d["Nl"], d["world"], rank, d["M"])
    local.setflags(write=False)
    seg.setflags(write=False)
    return local, seg
