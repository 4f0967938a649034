REGISTRY = {}

from .basic_controller import BasicMAC  # noqa: E402
from .non_shared_controller import NonSharedMAC  # noqa: E402

REGISTRY["basic_mac"] = BasicMAC
REGISTRY["non_shared_mac"] = NonSharedMAC
