from .remap import overlap_remap, overlap_remap_packed, RemapResult, revoke_map  # noqa: F401
from .interaction import Interaction  # noqa: F401
from .dataloader import CrossDomainDataloader, OverlapDataloader, DomainTrainLoader, FullSortEvalLoader  # noqa: F401
from .dataloader import NegSampleEvalLoader, eval_loader_for  # noqa: F401
from .popularity import train_item_counts, tail_items  # noqa: F401
