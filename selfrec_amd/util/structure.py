"""Small torch building blocks with the names of reference util/structure.py."""
import torch


class PointWiseFeedForward(torch.nn.Module):
    """x + Dropout(W2 act(W1 x + b1) + b2): two square Linear layers (``pwff.0`` / ``pwff.2``, the reference's state_dict
    keys), the activation between them, dropout on the second one's output, and the residual."""

    def __init__(self, hidden_units, dropout_rate, activation='relu'):
        super().__init__()
        act = {'relu': torch.nn.ReLU, 'gelu': torch.nn.GELU}[activation]()
        self.pwff = torch.nn.Sequential(
            torch.nn.Linear(hidden_units, hidden_units),
            act,
            torch.nn.Linear(hidden_units, hidden_units),
            torch.nn.Dropout(p=dropout_rate),
        )

    def forward(self, inputs):
        return self.pwff(inputs) + inputs
