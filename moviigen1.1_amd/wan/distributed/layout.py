"""SpLayout: which ranks a WanModel shares its token axis with, and how — one immutable value (WanModel.set_sp_layout installs it,
every stage of the forward reads it).  The `size` ranks of `group` own L/size consecutive tokens each; they form R Ulysses groups of U
consecutive ranks (all-to-all: the group's tokens x heads/U) and U rings of R strided ranks that rotate the K/V blocks of the groups:

    single      U = R = 1, no group
    ulysses     U = size, R = 1: the Ulysses group is `group`
    ring        U = 1, R = size: the ring is `group`
    hybrid      the reference CLI's `--ulysses_size U --ring_size R`

Every field holds its final value: no reader derives one from another.  A degree of 1 exchanges nothing, so outside the hybrid layout
(which creates all its groups) its group is None, unless `group` itself has one rank."""
import dataclasses

import torch.distributed as dist


def hybrid_rank_lists(P, U):
    """-> (uly_lists, ring_lists) of P ranks at Ulysses degree U: Ulysses group g is the ranks [g*U, (g+1)*U), ring u the ranks
    {u, u+U, u+2U, ...}; rank r is member r % U of Ulysses group r // U and member r // U of ring r % U."""
    if P % U:
        raise ValueError(f'the Ulysses degree {U} does not divide {P} ranks')
    R = P // U
    return [[g * U + u for u in range(U)] for g in range(R)], [[u + g * U for g in range(R)] for u in range(U)]


@dataclasses.dataclass(frozen=True, eq=False)       # eq=False: a layout is compared and hashed (the workspace key) by identity
class SpLayout:
    group: object       # all ranks that share the token axis (None: the single layout only), their number, this rank's index
    size: int
    rank: int
    U: int              # Ulysses degree, the group it exchanges in, this rank's index there
    uly_group: object
    uly_rank: int
    R: int              # ring degree, the group the K/V blocks rotate in, this rank's index there
    ring_group: object
    ring_rank: int

    def __post_init__(self):
        if self.U < 1 or self.R < 1 or self.U * self.R != self.size:
            raise ValueError('The number of ulysses_size and ring_size should be equal to the world size.')
        if not 0 <= self.rank < self.size or self.uly_rank != self.rank % self.U or self.ring_rank != self.rank // self.U:
            raise ValueError(f'rank {self.rank} of {self.size} at U = {self.U} is member {self.rank % self.U} of its Ulysses group and '
                             f'{self.rank // self.U} of its ring, not {self.uly_rank} and {self.ring_rank}')
        if self.group is None and self.size != 1:
            raise ValueError('only the single layout has no group')
        if self.U == self.size and self.uly_group is not self.group:
            raise ValueError('a Ulysses degree that spans the whole group exchanges in that group')
        if self.R == self.size and self.ring_group is not self.group:
            raise ValueError('a ring degree that spans the whole group rotates in that group')
        if (self.U > 1 and self.uly_group is None) or (self.R > 1 and self.ring_group is None):
            raise ValueError('a degree above 1 needs its group')

    @classmethod
    def single(cls):
        return cls(None, 1, 0, 1, None, 0, 1, None, 0)

    @classmethod
    def ulysses(cls, group=None):
        """Ulysses over all of `group` (default: WORLD); creates no group"""
        group = group if group is not None else dist.group.WORLD
        P, rank = dist.get_world_size(group), dist.get_rank(group)
        return cls(group, P, rank, P, group, rank, 1, group if P == 1 else None, 0)

    @classmethod
    def ring(cls, group=None):
        """ring attention over all of `group` (default: WORLD); creates no group"""
        group = group if group is not None else dist.group.WORLD
        P, rank = dist.get_world_size(group), dist.get_rank(group)
        return cls(group, P, rank, 1, group if P == 1 else None, 0, P, group, rank)

    @classmethod
    def hybrid(cls, U, R, group=None):
        """U x R over `group` (default: WORLD).  Every rank creates every group: the R Ulysses groups first, then the U rings."""
        P, rank = dist.get_world_size(group), dist.get_rank(group)
        U, R = int(U), int(R)
        if U * R != P:
            raise ValueError('The number of ulysses_size and ring_size should be equal to the world size.')
        glob = (lambda r: dist.get_global_rank(group, r)) if group is not None else (lambda r: r)
        uly_lists, ring_lists = hybrid_rank_lists(P, U)
        uly_groups = [dist.new_group([glob(r) for r in ranks]) for ranks in uly_lists]
        ring_groups = [dist.new_group([glob(r) for r in ranks]) for ranks in ring_lists]
        group = group if group is not None else dist.group.WORLD
        return cls(group, P, rank, U, group if U == P else uly_groups[rank // U], rank % U,
                   R, group if R == P else ring_groups[rank % U], rank // U)
