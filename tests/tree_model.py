"""Host model of the Poseidon Merkle tree: a heap of Python ints hashed with oracle/c's Poseidon.

Node p has the children 2p + 1 and 2p + 2; the leaves start at 2^depth - 1.  A write rehashes exactly the dirty parents,
level by level, one oracle call per level, so a ragged range of 40 000 leaves at depth 16 costs about two seconds.  The
model answers what the C ABI of the device tree promises (include/rln_amd.h, rlnamd_tree_*): the root, one path, and the
packed bytes of a range of paths.  It knows nothing of the product: the GPU tests compare the device tree with it, and
tests/test_tree_model_host.py compares it with oracle/pyref's FullMerkleTree."""
from oracle.c import binding as ob

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


class TreeModel:
    def __init__(self, depth, default_leaf=0):
        self.depth = depth
        zero = [default_leaf]                      # zero[h]: an all-default subtree of height h
        for _ in range(depth):
            zero.append(ob.poseidon_batch([[zero[-1], zero[-1]]])[0])
        self.nodes = []
        for level in range(depth + 1):             # level 0 is the root
            self.nodes += [zero[depth - level]] * (1 << level)
        self._node_bytes = None

    def copy(self):
        m = TreeModel.__new__(TreeModel)
        m.depth, m.nodes, m._node_bytes = self.depth, list(self.nodes), None
        return m

    def capacity(self):
        return 1 << self.depth

    # ------------------------------------------------------------------------------------------ writes
    def _write(self, updates):
        """{leaf index: value}: the leaves, then every dirty parent once, bottom-up"""
        cap = self.capacity()
        for i, v in updates.items():
            if not 0 <= i < cap:
                raise IndexError("leaf %d is outside a tree of depth %d" % (i, self.depth))
            if not 0 <= v < R:
                raise ValueError("leaf value is not a canonical field element")
        nodes = self.nodes
        for i, v in updates.items():
            nodes[cap - 1 + i] = v
        dirty = sorted(cap - 1 + i for i in updates)
        while dirty and dirty[0] > 0:
            parents = sorted({(n - 1) >> 1 for n in dirty})
            hashed = ob.poseidon_batch([[nodes[2 * p + 1], nodes[2 * p + 2]] for p in parents])
            for p, h in zip(parents, hashed):
                nodes[p] = h
            dirty = parents
        self._node_bytes = None

    def set_range(self, start, leaves):
        leaves = list(leaves)
        if start < 0 or start + len(leaves) > self.capacity():
            raise IndexError("TooManySet")
        self._write({start + i: v for i, v in enumerate(leaves)})

    def set(self, index, leaf):
        self.set_range(index, [leaf])

    def set_leaves(self, updates):
        """[(index, leaf)] in any order; a later entry for an index wins"""
        self._write(dict(updates))

    def fill_sequential(self, start, n, first_value):
        """leaf start + i <- first_value + i as a 64-bit counter"""
        self.set_range(start, [(first_value + i) & 0xFFFFFFFFFFFFFFFF for i in range(n)])

    # ------------------------------------------------------------------------------------------ reads
    def root(self):
        return self.nodes[0]

    def get(self, index):
        if not 0 <= index < self.capacity():
            raise IndexError("InvalidLeaf")
        return self.nodes[self.capacity() - 1 + index]

    def proof(self, index):
        """-> (siblings bottom-up, bits; bit = 1 when the node on the path is a right child, the even heap index)"""
        if not 0 <= index < self.capacity():
            raise IndexError("InvalidLeaf")
        n = self.capacity() - 1 + index
        elems, bits = [], []
        while n > 0:
            right = n % 2 == 0
            elems.append(self.nodes[n - 1 if right else n + 1])
            bits.append(1 if right else 0)
            n = (n - 1) >> 1
        return elems, bits

    def proofs_bytes(self, first, count):
        """the paths of leaves [first, first + count) as the C ABI packs them -> (count * depth * 32 bytes of canonical
        little-endian siblings, count * depth bit bytes), proof-major and bottom-up inside a proof"""
        if first < 0 or count < 0 or first + count > self.capacity():
            raise IndexError("InvalidLeaf")
        if self._node_bytes is None:
            self._node_bytes = [v.to_bytes(32, "little") for v in self.nodes]
        nb, d, cap = self._node_bytes, self.depth, self.capacity()
        # with heap indices counted from 1 the ancestor of leaf i at height l is (cap + i) >> l, its sibling differs in
        # the lowest bit, and a right child is odd
        ones = range(cap + first, cap + first + count)
        elems = b"".join(nb[((one >> l) ^ 1) - 1] for one in ones for l in range(d))
        bits = bytes((one >> l) & 1 for one in ones for l in range(d))
        return elems, bits
