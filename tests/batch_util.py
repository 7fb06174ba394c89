"""TEST INFRASTRUCTURE for the batched surface on a machine without a GPU: the host restatement of the one method of the batched path
that touches the engine (``HIPnnUNetPredictor._sliding_window_batch``) as a loop over ``HostLogicPredictor``'s per-case path, and the
model that uses it."""
import numpy as np

from tests.host_predictor import HostLogicPredictor
from tests.surface_util import HostModel, synthetic_model


class HostBatchPredictor(HostLogicPredictor):
    def _sliding_window_batch(self, list_of_data, fold: int = 0, want_seg: bool = False):
        out = []
        for i, d in enumerate(list_of_data):
            try:
                lg = self.predict_sliding_window_return_logits(np.asarray(d, dtype=np.float32), fold)
            except Exception as ex:
                raise RuntimeError(f'input {i}: {ex}') from ex
            # the device predicate: sigmoid(float(half logit)) > 0.5 <=> the half value exceeds 0 (export.py)
            out.append((lg.astype(np.float32) > 1.5 * 2.0 ** -24).astype(np.uint8) if want_seg else lg)
        return out


class HostBatchModel(HostModel):
    def _make_predictor(self, kw):
        return HostBatchPredictor(network=self._config['oracle_network'], **kw)


def synthetic_batch_model(*a, **kw):
    m, arch, sd = synthetic_model(*a, network=True, **kw)
    return HostBatchModel(m._config), arch, sd
